"""Python host-side mirror of ORB_SLAM2::Tracking::TrackWithMotionModel (reference orb_object_slam/src/Tracking.cc:1276-1354: UpdateLastFrame, the frame-to-frame
SearchByProjection with its stereo branch and the retry at twice the radius, PoseOptimization, the outlier loop) and of Tracking::TrackLocalMap (:1356-1416) and what it calls: UpdateLocalMap (:2730-2738) with
UpdateLocalKeyFrames (:2766-2874) and UpdateLocalPoints (:2740-2764), SearchLocalPoints (:2673-2728), Optimizer::PoseOptimization and the statistics loop (:1372-1397).

The map is a table of points and a table of key frames in flat arrays (`Map` below); a frame is a `TrackedFrame`.  What the reference keeps as pointers are indices into those
tables, -1 for NULL.  The search, the frustum test, the local point list and the pose run on the device; the walk over the key-frame graph, the loop over the frame's own
points and the statistics over N flags stay on the host."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, lib, ptr
from .matcher import ORBmatcher
from .optimizer import PoseOptimization


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _u8(a):
    return np.ascontiguousarray(a, np.uint8)


def pose7_to_Tcw(p):
    """The 3x4 float pose of (t, qx, qy, qz, qw): what Frame::SetPose receives after PoseOptimization (the quaternion's rotation matrix in double, stored as float)."""
    x, y, z, w = [np.float64(v) for v in p[3:7]]
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)
    return np.concatenate([Rm, np.asarray(p[:3], np.float64).reshape(3, 1)], axis=1).astype(np.float32)


def Tcw_to_pose7(T):
    """(t, qx, qy, qz, qw) of a 3x4 pose, what PoseOptimization starts from: the rotation's unit quaternion with qw >= 0, every step a double in a fixed order (the C++ mirror,
    host/tracking.hpp, computes the same bits)."""
    T = np.asarray(T, np.float64).reshape(-1)[:12].reshape(3, 4)
    R = [[float(T[i, j]) for j in range(3)] for i in range(3)]
    tr = R[0][0] + R[1][1] + R[2][2]
    q = [0.0, 0.0, 0.0, 0.0]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [(R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s, 0.25 * s]
    else:
        i = 0
        if R[1][1] > R[i][i]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        s = math.sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0) * 2
        q[i] = 0.25 * s; q[3] = (R[k][j] - R[j][k]) / s; q[j] = (R[j][i] + R[i][j]) / s; q[k] = (R[k][i] + R[i][k]) / s
    if q[3] < 0:
        q = [-v for v in q]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([float(T[0, 3]), float(T[1, 3]), float(T[2, 3]), q[0] / n, q[1] / n, q[2] / n, q[3] / n], np.float64)


def track_local_points(ctx, kf_off, kf_mp, skip):
    """Tracking::UpdateLocalPoints (cs_track_local_points): the concatenated map-point lists of the local key frames -> mvpLocalMapPoints."""
    off, mp, sk = _i32(kf_off), _i32(kf_mp), _u8(skip)
    out = np.zeros(max(min(int(off[-1]), len(sk)), 1), np.int32); n = C.c_int()
    check(ctx.ptr, lib().cs_track_local_points(ctx.ptr, len(off) - 1, ptr(off), ptr(mp), len(sk), ptr(sk), ptr(out), C.byref(n)), "cs_track_local_points")
    return out[:n.value].copy()


def track_local_keyframes(frame_mp, mp_skip, obs_off, obs_kf, kf_bad, cov_off, cov_kf, child_off, child_kf, parent):
    """Tracking::UpdateLocalKeyFrames (cs_track_local_keyframes, host) -> (mvpLocalKeyFrames or None when no key frame received a vote, pKFmax or -1)."""
    fm, ms, oo, ok, kb = _i32(frame_mp), _u8(mp_skip), _i32(obs_off), _i32(obs_kf), _u8(kf_bad)
    co, ck, ho, hk, pa = _i32(cov_off), _i32(cov_kf), _i32(child_off), _i32(child_kf), _i32(parent)
    out = np.zeros(max(len(kb), 1), np.int32); n = C.c_int(); mx = C.c_int()
    r = lib().cs_track_local_keyframes(len(fm), ptr(fm), len(ms), ptr(ms), ptr(oo), ptr(ok), len(kb), ptr(kb), ptr(co), ptr(ck),
                                       ptr(ho), ptr(hk), ptr(pa), ptr(out), C.byref(n), C.byref(mx))
    check(None, r, "cs_track_local_keyframes")
    return (None if n.value < 0 else out[:n.value].copy()), mx.value


class Map:
    """The point and key-frame tables the tracking thread reads.  Points: world_pos, normal, min_distance (mfMinDistance), max_distance, desc, bad (isBad), dynamic (is_dynamic),
    n_obs (Observations()), obs_off / obs_kf (the key frames of GetObservations()), last_frame_seen, visible, found.  Key frames: kf_off / kf_mp (GetMapPointMatches()), kf_bad,
    cov_off / cov_kf (mvpOrderedConnectedKeyFrames), child_off / child_kf, parent."""

    def __init__(self, **arrays):
        self.__dict__.update(arrays)
        n = len(self.bad)
        for name in ("last_frame_seen", "visible", "found"):
            if not hasattr(self, name):
                setattr(self, name, np.full(n, -1, np.int64) if name == "last_frame_seen" else np.zeros(n, np.int64))
        if not hasattr(self, "dynamic"):
            self.dynamic = np.zeros(n, np.uint8)

    def append_points(self, world_pos, desc):
        """`new MapPoint(x3D, mpMap, &mLastFrame, i)` for each row (Tracking.cc:1259): points without observations behind the table's last; returns their indices.  The
        descriptor is the creating key point's (MapPoint.cc:64); the fields a temporal point never has read (normal, distances) are zero."""
        k, n = len(world_pos), len(self.bad)
        grow = lambda a, tail: np.concatenate([a, tail.astype(a.dtype)])
        self.world_pos = grow(np.asarray(self.world_pos), np.asarray(world_pos, np.float32).reshape(k, 3))
        self.normal = grow(np.asarray(self.normal), np.zeros((k, 3)))
        self.desc = grow(np.asarray(self.desc), np.asarray(desc, np.uint8).reshape(k, 32))
        for name in ("min_distance", "max_distance", "bad", "dynamic", "n_obs", "visible", "found"):
            setattr(self, name, grow(np.asarray(getattr(self, name)), np.zeros(k)))
        self.last_frame_seen = grow(self.last_frame_seen, np.full(k, -1))
        self.obs_off = grow(np.asarray(self.obs_off), np.full(k, np.asarray(self.obs_off)[-1]))
        return np.arange(n, n + k, dtype=np.int64)


class TrackedFrame:
    """mCurrentFrame as TrackLocalMap reads and writes it: mnId, mvKeysUn, mDescriptors, the image bounds, mvpMapPoints (indices, -1), mvbOutlier, the pose (Rcw, tcw, Ow as float32),
    intr = (fx, fy, cx, cy, mbf), mfLogScaleFactor, mvScaleFactors, mvInvLevelSigma2, mvuRight (optional), KeysStatic (optional)."""

    def __init__(self, mnId, keysUn, desc, bounds, mvpMapPoints, Rcw, tcw, Ow, intr, log_scale_factor, scale_factors, inv_level_sigma2, pose7, u_right=None, keys_static=None):
        self.mnId, self.keysUn, self.desc, self.bounds = mnId, keysUn, desc, bounds
        self.mvpMapPoints = np.array(mvpMapPoints, np.int32)
        self.mvbOutlier = np.zeros(len(keysUn), np.uint8)
        self.Rcw, self.tcw, self.Ow = Rcw, tcw, Ow
        self.intr, self.log_scale_factor, self.scale_factors, self.inv_level_sigma2 = intr, log_scale_factor, scale_factors, inv_level_sigma2
        self.pose7 = np.asarray(pose7, np.float64)
        self.u_right = np.full(len(keysUn), -1.0, np.float32) if u_right is None else np.asarray(u_right, np.float32)
        self.has_u_right = u_right is not None  # a stereo / RGB-D frame: the searches apply the mvuRight tests
        self.u_right_device = None              # a device address of the same mvuRight (RGBDAssociator.device_frame, StereoMatcher.device_pair): set_u_right then takes it from there
        self.keys_static = keys_static

    def SetPose(self, Tcw):
        """Frame::SetPose / UpdatePoseMatrices (Frame.cc:320-344) for a 3x4 float pose: mRcw, mtcw, mOw = -mRcw.t() * mtcw (one gemm per row: double accumulation, one rounding)."""
        T = np.asarray(Tcw, np.float32).reshape(-1)[:12].reshape(3, 4)
        self.Rcw, self.tcw = T[:, :3].copy(), T[:, 3].copy()
        self.Ow = np.array([np.float32(-sum(np.float64(T[k, r]) * np.float64(T[k, 3]) for k in range(3))) for r in range(3)], np.float32)

    @property
    def Tcw(self):
        return np.concatenate([np.asarray(self.Rcw, np.float32).reshape(3, 3), np.asarray(self.tcw, np.float32).reshape(3, 1)], axis=1)


class LastFrame:
    """mLastFrame as TrackWithMotionModel reads it: mvKeysUn (level and angle), mDescriptors, mvpMapPoints (indices, -1), mvbOutlier, mTcw (3x4 float32), mvDepth, and whether it
    is the reference key frame's own frame (UpdateLastFrame then creates nothing, Tracking.cc:1215).  rgbd: an RGBDAssociator that still holds this frame alone on the device."""

    def __init__(self, keysUn, desc, mvpMapPoints, Tcw, mvDepth=None, mvbOutlier=None, is_keyframe=False, rgbd=None):
        self.keysUn, self.desc, self.mvpMapPoints = keysUn, np.asarray(desc, np.uint8), np.array(mvpMapPoints, np.int64)
        self.Tcw = np.asarray(Tcw, np.float32).reshape(-1)[:12].reshape(3, 4)
        self.mvDepth = mvDepth
        self.mvbOutlier = np.zeros(len(keysUn), np.uint8) if mvbOutlier is None else np.asarray(mvbOutlier, np.uint8)
        self.is_keyframe, self.rgbd = is_keyframe, rgbd


class Tracking:
    STEREO, MONOCULAR, RGBD = 1, 0, 2  # System::eSensor

    def __init__(self, ctx=None, device=0, sensor=0, whether_dynamic_object=False, whether_detect_object=False, mbOnlyTracking=False, mMaxFrames=30, **matcher_kw):
        self.ctx = ctx or _lib.Context(device)
        self.mSensor, self.whether_dynamic_object, self.whether_detect_object, self.mbOnlyTracking, self.mMaxFrames = sensor, whether_dynamic_object, whether_detect_object, mbOnlyTracking, mMaxFrames
        self.matcher = ORBmatcher(0.8, True, ctx=self.ctx, **matcher_kw)  # :2719
        self.mvpLocalKeyFrames = np.zeros(0, np.int32)
        self.mvpLocalMapPoints = np.zeros(0, np.int32)
        self.mpReferenceKF = -1
        self.mnLastRelocFrameId = -10 ** 9
        self.mnMatchesInliers = 0
        self.last_search = None

    def _skip(self, m):
        return (m.bad != 0) | ((m.dynamic != 0) if self.whether_dynamic_object else False)

    def UpdateLocalKeyFrames(self, F, m):
        mp = F.mvpMapPoints
        has = mp >= 0
        F.mvpMapPoints[has & (m.bad[np.where(has, mp, 0)] != 0)] = -1  # :2783-2786
        local, kfmax = track_local_keyframes(F.mvpMapPoints, self._skip(m), m.obs_off, m.obs_kf, m.kf_bad, m.cov_off, m.cov_kf, m.child_off, m.child_kf, m.parent)
        if local is not None:
            self.mvpLocalKeyFrames = local
            if kfmax >= 0:
                self.mpReferenceKF = kfmax
        return self.mvpLocalKeyFrames

    def UpdateLocalPoints(self, F, m):
        off = np.zeros(len(self.mvpLocalKeyFrames) + 1, np.int32)
        lens = (m.kf_off[1:] - m.kf_off[:-1])[self.mvpLocalKeyFrames]
        off[1:] = np.cumsum(lens)
        mp = np.concatenate([m.kf_mp[m.kf_off[j]:m.kf_off[j + 1]] for j in self.mvpLocalKeyFrames]) if len(lens) else np.zeros(0, np.int32)
        self.mvpLocalMapPoints = track_local_points(self.ctx, off, mp, self._skip(m))
        return self.mvpLocalMapPoints

    def UpdateLocalMap(self, F, m):
        self.UpdateLocalKeyFrames(F, m)
        return self.UpdateLocalPoints(F, m)

    def SearchLocalPoints(self, F, m):
        mp = F.mvpMapPoints
        has = mp >= 0
        F.mvpMapPoints[has & (m.bad[np.where(has, mp, 0)] != 0)] = -1  # :2681-2684
        own = F.mvpMapPoints[(F.mvpMapPoints >= 0)]
        own = own[m.dynamic[own] == 0]  # :2687
        np.add.at(m.visible, own, 1)
        m.last_frame_seen[own] = F.mnId
        lp = self.mvpLocalMapPoints
        skip = (m.last_frame_seen[lp] == F.mnId) | (m.bad[lp] != 0) | (m.dynamic[lp] != 0)  # :2702-2707
        th = 1
        if self.mSensor == self.RGBD:
            th = 3
        if F.mnId < self.mnLastRelocFrameId + 2:
            th = 5
        held = F.mvpMapPoints >= 0
        tb = np.zeros(len(F.keysUn), np.uint8)
        tb[held] = m.n_obs[F.mvpMapPoints[held]] > 0  # :96-98
        if F.keys_static is not None:
            tb |= (np.asarray(F.keys_static) == 0).astype(np.uint8)  # :101
        self.matcher.set_frame(F.keysUn, F.desc, F.bounds)
        stereo = self.mSensor != self.MONOCULAR and getattr(F, "has_u_right", False)  # ORBmatcher.cc:104-109: a frame with right coordinates tests them
        if stereo:
            self.matcher.set_u_right(F.u_right if F.u_right_device is None else int(F.u_right_device), n=len(F.keysUn))
        fx, fy, cx, cy, bf = F.intr
        r = self.matcher.SearchLocalPoints(F.Rcw, F.tcw, F.Ow, m.world_pos[lp], m.normal[lp], m.min_distance[lp], m.max_distance[lp], skip, m.n_obs[lp] > 0, m.desc[lp], fx, fy, cx, cy, bf,
                                           F.log_scale_factor, F.scale_factors, float(th), 0.5, tb, **({"stereo": True} if stereo else {}))
        np.add.at(m.visible, lp[r["in_view"] != 0], 1)  # :2712
        got = r["train_match"] >= 0
        F.mvpMapPoints[got] = lp[r["train_match"][got]]  # :136
        self.last_search = r
        return r

    def TrackLocalMap(self, F, m):
        self.UpdateLocalMap(F, m)
        self.SearchLocalPoints(F, m)
        idx = np.nonzero(F.mvpMapPoints >= 0)[0]
        mp = F.mvpMapPoints[idx]
        obs = np.stack([F.keysUn["x"][idx], F.keysUn["y"][idx], F.u_right[idx]], axis=1).astype(np.float64) if len(idx) else np.zeros((0, 3))
        fr = {"Xw": m.world_pos[mp].astype(np.float64), "obs": obs, "inv_sigma2": np.asarray(F.inv_level_sigma2, np.float32)[F.keysUn["octave"][idx]].astype(np.float64),
              "intr": np.asarray(F.intr, np.float32).astype(np.float64), "pose": F.pose7}  # (the Frame's intrinsics are floats)
        pose, flags, _ = PoseOptimization([fr], ctx=self.ctx)[0]  # :1366
        F.pose7 = pose
        F.mvbOutlier[:] = 0
        F.mvbOutlier[idx] = flags
        self.mnMatchesInliers = 0
        for i, p in zip(idx, mp):  # :1372-1397
            if not F.mvbOutlier[i]:
                if self.whether_dynamic_object and m.dynamic[p]:
                    continue
                m.found[p] += 1
                if not self.mbOnlyTracking:
                    if m.n_obs[p] > 0:
                        self.mnMatchesInliers += 1
                else:
                    self.mnMatchesInliers += 1
            elif self.mSensor == self.STEREO:
                F.mvpMapPoints[i] = -1
        if F.mnId < self.mnLastRelocFrameId + self.mMaxFrames and self.mnMatchesInliers < 50:  # :1402
            return False
        return self.mnMatchesInliers >= (20 if self.whether_detect_object else 30)  # :1405-1415

    def TrackWithMotionModel(self, F, last, m, predicted_pose, K4=None, mThDepth=0.0):
        """Tracking::TrackWithMotionModel (Tracking.cc:1276-1354).  F: the current TrackedFrame; last: the LastFrame; m: the Map; predicted_pose = mVelocity * mLastFrame.mTcw
        (3x4) -- the velocity model stays the caller's, as does the SearchByTracking* step of :1306-1312 (cube_slam_amd.klt).  K4 / mThDepth: what UpdateLastFrame's close-point rule
        reads; the "visual odometry" points it creates are appended to the Map (Map.append_points) and to self.mlpTemporalPoints (UpdateLastFrame keeps that list).  Leaves nmatches, nmatchesMap (and mbVO under
        mbOnlyTracking) on self, the matches and the optimised pose on F; returns what the reference returns."""
        # :1282 UpdateLastFrame
        mp, ids, x3D = self.UpdateLastFrame(last.mvDepth, last.keysUn, last.mvpMapPoints, m.n_obs, last.Tcw, K4, mThDepth, next_point_id=len(m.bad), last_frame_is_keyframe=last.is_keyframe,
                                            rgbd=last.rgbd)
        if len(ids):
            created = np.array([int(np.nonzero(mp == i)[0][0]) for i in ids], np.int64)
            got = m.append_points(x3D, last.desc[created])
            assert got.tolist() == list(ids)
        last.mvpMapPoints = mp
        # :1284-1287
        F.SetPose(predicted_pose)
        F.pose7 = Tcw_to_pose7(F.Tcw)
        F.mvpMapPoints[:] = -1
        th = 7 if self.mSensor == self.STEREO else 15  # :1293-1296
        bMono = self.mSensor == self.MONOCULAR
        has = mp >= 0
        pm = np.where(has, mp, 0)
        valid = has & (last.mvbOutlier == 0) & (m.dynamic[pm] == 0)  # :1400-1405
        tb = None if F.keys_static is None else (np.asarray(F.keys_static) == 0).astype(np.uint8)  # :1456 (the frame holds no map point yet, :1451)
        fx, fy, cx, cy, bf = [float(np.float32(a)) for a in F.intr]
        mb = float(np.float32(np.float32(bf) / np.float32(fx)))  # Frame.cc:141
        self.matcher.mbCheckOrientation = True  # ORBmatcher matcher(0.9, true), :1278
        self.matcher.set_frame(F.keysUn, F.desc, F.bounds)
        if not bMono:
            self.matcher.set_u_right(F.u_right if F.u_right_device is None else int(F.u_right_device), n=len(F.keysUn))

        def search(radius):
            tm, n = self.matcher.SearchByProjectionFrame(m.world_pos[pm], valid, m.n_obs[pm] > 0, m.desc[pm], last.keysUn["octave"], last.keysUn["angle"], F.Tcw, fx, fy, cx, cy,
                                                         F.scale_factors, float(radius), tb, bMono=bMono, Tlw=last.Tcw, bf=bf, mb=mb)
            F.mvpMapPoints[:] = np.where(tm >= 0, mp[np.maximum(tm, 0)], -1)
            return n
        nmatches = search(th)
        self.retried = nmatches < 20
        if nmatches < 20:  # :1300-1304
            nmatches = search(2 * th)
        self.nmatches, self.nmatchesMap = nmatches, 0
        if nmatches < 20:  # :1314-1318
            return False
        idx = np.nonzero(F.mvpMapPoints >= 0)[0]
        pts = F.mvpMapPoints[idx]
        obs = np.stack([F.keysUn["x"][idx], F.keysUn["y"][idx], F.u_right[idx]], axis=1).astype(np.float64)
        fr = {"Xw": m.world_pos[pts].astype(np.float64), "obs": obs, "inv_sigma2": np.asarray(F.inv_level_sigma2, np.float32)[F.keysUn["octave"][idx]].astype(np.float64),
              "intr": np.asarray(F.intr, np.float32).astype(np.float64), "pose": F.pose7}
        pose, flags, _ = PoseOptimization([fr], ctx=self.ctx)[0]  # :1321
        F.pose7 = pose
        F.SetPose(pose7_to_Tcw(pose))  # Optimizer.cc:468-469
        F.mvbOutlier[:] = 0
        F.mvbOutlier[idx] = flags
        self.last_outliers = F.mvbOutlier.copy()
        nmatchesMap = 0
        for i, p in zip(idx, pts):  # :1326-1345
            if F.mvbOutlier[i]:
                F.mvpMapPoints[i] = -1
                F.mvbOutlier[i] = 0
                m.last_frame_seen[p] = F.mnId  # (mbTrackInView = false: the search's own field)
                nmatches -= 1
            elif m.n_obs[p] > 0 and not (self.whether_dynamic_object and m.dynamic[p]):
                nmatchesMap += 1
        self.nmatches, self.nmatchesMap = nmatches, nmatchesMap
        if self.mbOnlyTracking:  # :1347-1351
            self.mbVO = nmatchesMap < 10
            return nmatches > 20
        return nmatchesMap >= 10

    def UpdateLastFrame(self, mvDepth, keysUn, mvpMapPoints, observations, Tcw, K4, mThDepth, next_point_id, last_frame_is_keyframe=False, rgbd=None, host=False):
        """The point creation of Tracking::UpdateLastFrame (Tracking.cc:1215-1273) over index tables.  mvDepth / keysUn / mvpMapPoints (-1 = NULL) are the last
        frame's, observations[p] = MapPoint::Observations() of map point p, Tcw [3, 4] the pose the caller has set (:1213), next_point_id = MapPoint::nNextId.  The
        created "visual odometry" points take the ids next_point_id, next_point_id + 1, ... in creation order, fill their slots and are appended to mlpTemporalPoints.
        Returns (mvpMapPoints afterwards, the ids created, their positions [k, 3]).  rgbd: an RGBDAssociator whose last call left this frame (alone) on the device --
        depth and key points are then not uploaded; host=True: the statement on the host."""
        from .rgbd import CS_CLOSE_POINTS_NEAREST, ClosePoints
        mp = np.array(mvpMapPoints, np.int64)
        temporal = self.__dict__.setdefault("mlpTemporalPoints", [])
        if last_frame_is_keyframe or self.mSensor == self.MONOCULAR:  # :1215
            return mp, [], np.zeros((0, 3), np.float32)
        obs = np.asarray(observations)
        need_new = ((mp < 0) | (obs[np.maximum(mp, 0)] < 1)).astype(np.uint8)  # !pMP || pMP->Observations() < 1
        if rgbd is not None and not host:
            r = rgbd.close_points(need_new, np.asarray(Tcw, np.float32)[None], K4, mThDepth, CS_CLOSE_POINTS_NEAREST)[0]
        else:
            r = ClosePoints(mvDepth, keysUn, need_new, Tcw, K4, mThDepth, CS_CLOSE_POINTS_NEAREST, ctx=None if host else self.ctx)
        ids = list(range(int(next_point_id), int(next_point_id) + len(r["new_idx"])))
        mp[r["new_idx"]] = ids  # mLastFrame.mvpMapPoints[i] = pNewMP
        temporal.extend(ids)    # mlpTemporalPoints.push_back(pNewMP)
        return mp, ids, r["new_x3D"]

    def StereoInitializationPoints(self, mvDepth, keysUn, Tcw, K4, host=False):
        """The loop of Tracking::StereoInitialization (Tracking.cc:804-819): (the key points with z > 0 in index order, Frame::UnprojectStereo of each).  The test
        mCurrentFrame.N > 500 (:786), the key frame and everything done with `new MapPoint` stay the caller's."""
        from .rgbd import CS_CLOSE_POINTS_ALL, ClosePoints
        r = ClosePoints(mvDepth, keysUn, None, Tcw, K4, 0.0, CS_CLOSE_POINTS_ALL, ctx=None if host else self.ctx)
        return r["new_idx"], r["new_x3D"]

    def TrackHarrisFeatures(self, last_gray, current_gray, mvKeysHarris_pt, mvpMapPointsHarris, objmask_img, ctx=None):
        """The dynamic branch of Tracking::TrackWithMotionModel with use_dynamic_klt_features (Tracking.cc:1308-1311): ORBmatcher::SearchByTrackingHarris from the
        last frame to the current one.  Returns the current frame's (mvKeysHarris pt, mvpMapPointsHarris, keypoint_associate_objectID_harris) and the search's dict.
        ctx=None: on the host."""
        from .klt import SearchByTrackingHarris
        r = SearchByTrackingHarris(np.stack([np.asarray(last_gray, np.uint8), np.asarray(current_gray, np.uint8)]), [(0, 1)], [mvKeysHarris_pt], [objmask_img], ctx=ctx)[0]
        return r["pts"], np.asarray(mvpMapPointsHarris)[r["kept"]], r["object_id"], r

    def CreateNewHarrisFeatures(self, gray, objmask_img, mvKeysHarris_pt, mvpMapPointsHarris, observations, object_id_harris, K4, Twc, cuboid_depth, next_point_id=0, ctx=None,
                                tracker=None, frame=0):
        """The new-feature loop of Tracking::CreateNewKeyFrame with use_dynamic_klt_features (Tracking.cc:2258-2337).  mvKeysHarris_pt / mvpMapPointsHarris /
        object_id_harris describe the current frame's tracked Harris points (a map point of None or < 0 is no point), observations[i] = Observations() of point i,
        cuboid_depth = the camera z of the key frame's local cuboids.  Returns the extended (mvKeysHarris pt, mvpMapPointsHarris, keypoint_associate_objectID_harris),
        the new points' positions and the call's dict; the new map points get the ids next_point_id, next_point_id + 1, ...  `new MapPoint` and SetupSimpleMapPoints
        stay the caller's.  ctx=None: on the host; tracker: a KLTTracker that holds the frame at index `frame`."""
        from .klt import NewHarrisFeatures
        pts = np.asarray(mvKeysHarris_pt, np.float32).reshape(-1, 2)
        mps = np.asarray([-1 if m is None else m for m in mvpMapPointsHarris], np.int64).reshape(-1)
        ids = np.asarray(object_id_harris, np.int32).reshape(-1)
        has = mps >= 0  # `pMP && pMP->is_dynamic`: every Harris map point is dynamic
        args = ([np.asarray(objmask_img, np.uint8)], [pts[has]], [np.asarray(observations, np.int32).reshape(-1)[has]], K4, np.asarray(Twc, np.float32).reshape(-1)[None, :12],
                [cuboid_depth])
        r = (tracker.new_harris_features([frame], *args) if tracker is not None else NewHarrisFeatures(np.asarray(gray, np.uint8), *args, ctx=ctx))[0]
        new_ids = np.arange(int(next_point_id), int(next_point_id) + len(r["pts"]), dtype=np.int64)
        return np.concatenate([pts, r["pts"]]), np.concatenate([mps, new_ids]), np.concatenate([ids, r["object_id"]]), r["x3D"], r

    def close(self):
        self.matcher.close()
