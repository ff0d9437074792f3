"""Python host-side mirror of ORB_SLAM2::ORBmatcher's Hamming searches (reference orb_object_slam/include/ORBmatcher.h:43-89)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Handle, check, lib, ptr
from .orb import KEYPOINT_DTYPE


class ORBmatcher(Handle):
    HANDLE, DESTROY = "_m", "cs_matcher_destroy"
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, checkOri=True, ctx=None, device=0, max_keypoints=8192, max_queries=16384, max_candidates=4000000):
        self.ctx = ctx or _lib.Context(device)
        self.mfNNratio, self.mbCheckOrientation = nnratio, checkOri
        self._m = C.c_void_p()
        check(self.ctx.ptr, lib().cs_matcher_create(self.ctx.ptr, max_keypoints, max_queries, max_candidates, C.byref(self._m)), "cs_matcher_create")
        self.N = 0
        self.has_u_right = False
        self.last_direction = 0

    def set_frame(self, keysUn, descriptors, bounds):
        """The frame that is searched (CurrentFrame / F / F2): mvKeysUn, mDescriptors, (mnMinX, mnMaxX, mnMinY, mnMaxY).  Detaches mvuRight (set_u_right)."""
        k = np.ascontiguousarray(keysUn, KEYPOINT_DTYPE); d = np.ascontiguousarray(descriptors, np.uint8)
        self.N = len(k)
        self.has_u_right = False
        check(self.ctx.ptr, lib().cs_matcher_set_frame(self.ctx.ptr, self._m, ptr(k), ptr(d), self.N, *bounds), "cs_matcher_set_frame")

    def set_frame_from_orb(self, orb, frame, K4, dist5=None, bounds=None, width=None, height=None, read_keys=True):
        """Frame post-processing on the device: keypoints / descriptors of frame `frame` of the extractor's last run are undistorted
        (Frame::UndistortKeyPoints) and binned (AssignFeaturesToGrid) without leaving HBM.  Returns (mvKeysUn, bounds); read_keys=False: (None, bounds) and the
        frame's key points stay on the device (every search but SearchForInitialization's vbPrevMatched update works from the device copy)."""
        k4 = np.ascontiguousarray(K4, np.float32)
        d5 = None if dist5 is None else np.ascontiguousarray(dist5, np.float32)
        if bounds is None:
            bounds = frame_image_bounds(width, height, k4, d5)
        out = np.zeros(max(orb.cap, 1), KEYPOINT_DTYPE); n = C.c_int()
        check(self.ctx.ptr, lib().cs_matcher_set_frame_from_orb(self.ctx.ptr, self._m, orb._e, int(frame), ptr(k4), ptr(d5),
                                                                *[float(b) for b in bounds], ptr(out) if read_keys else None, C.byref(n)),
              "cs_matcher_set_frame_from_orb")
        self.N = n.value
        self.has_u_right = False
        return (out[:n.value].copy() if read_keys else None), tuple(float(b) for b in bounds)

    def set_u_right(self, u_right, n=None):
        """CurrentFrame.mvuRight for the stereo searches of the frame set last (cs_matcher_set_u_right): a float array of N values, or a device address (int, with n) as
        StereoMatcher.device_pair / RGBDAssociator.device_frame hand out -- then nothing passes through the host.  The next set_frame* detaches it."""
        if isinstance(u_right, (int, np.integer)):
            check(self.ctx.ptr, lib().cs_matcher_set_u_right(self.ctx.ptr, self._m, C.cast(C.c_void_p(int(u_right)), C.POINTER(C.c_float)), self.N if n is None else int(n), 1), "cs_matcher_set_u_right")
        else:
            ur = np.ascontiguousarray(u_right, np.float32)
            check(self.ctx.ptr, lib().cs_matcher_set_u_right(self.ctx.ptr, self._m, ptr(ur if len(ur) else np.zeros(1, np.float32)), len(ur), 0), "cs_matcher_set_u_right")
        self.has_u_right = True

    def SearchByTrackingHarris(self, last_gray, current_gray, mvKeysHarris_pt, objmask_img):
        """ORBmatcher::SearchByTrackingHarris (ORBmatcher.cc:1524-1580) for one pair of gray frames on this matcher's context: a dict of kept (indices into the last
        frame's mvKeysHarris / mvpMapPointsHarris), pts (the current frame's mvKeysHarris), object_id, goodmatches, n_mask_outside, featuresklt_lastframe /
        featuresklt_thisframe, status, err.  Many pairs in one call: cube_slam_amd.klt.KLTTracker.search_by_tracking_harris."""
        from .klt import SearchByTrackingHarris
        return SearchByTrackingHarris(np.stack([np.asarray(last_gray, np.uint8), np.asarray(current_gray, np.uint8)]), [(0, 1)], [mvKeysHarris_pt], [objmask_img], ctx=self.ctx)[0]

    def SearchByTracking(self, last_gray, current_gray, last_keys, eligible, object_id, numobject, th, scale_factors, keys_static=None, had_map_point=None, tracker=None,
                         frames=(0, 1)):
        """ORBmatcher::SearchByTracking (ORBmatcher.cc:1582-1725) against this matcher's frame (the current frame): see cube_slam_amd.klt.SearchByTracking."""
        from .klt import SearchByTracking
        return SearchByTracking(last_gray, current_gray, last_keys, eligible, object_id, numobject, th, scale_factors, None, None, keys_static, had_map_point, matcher=self,
                                tracker=tracker, frames=frames)

    def last_candidate_stats(self):
        q, c = C.c_int(), C.c_long()
        if lib().cs_matcher_last_counts(self._m, C.byref(q), C.byref(c)) != 0:
            return None
        return {"queries": q.value, "candidates": c.value}

    def GetFeaturesInArea(self, x, y, r, minLevel=-1, maxLevel=-1):
        out = np.zeros(max(self.N, 1), np.int32); n = C.c_int()
        check(self.ctx.ptr, lib().cs_matcher_features_in_area(self.ctx.ptr, self._m, x, y, r, minLevel, maxLevel,
                                                              ptr(out), len(out), C.byref(n)), "cs_matcher_features_in_area")
        return out[:n.value].copy()

    def SearchByProjectionFrame(self, world_pos, valid, blocks, mp_desc, last_octave, last_angle, Tcw, fx, fy, cx, cy, scale_factors, th, train_blocked=None, bMono=True, Tlw=None,
                                bf=0.0, mb=0.0):
        """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (ORBmatcher.cc:1373-1522) against the frame set last: (train_match, nmatches).  bMono=False: the
        stereo branch -- Tlw = LastFrame.mTcw, bf = mbf, mb = the baseline, mvuRight from set_u_right; the direction it took (0 neither, 1 forward, 2 backward) is left in
        last_direction."""
        if not bMono:
            return self.SearchByProjectionFrameStereo(world_pos, valid, blocks, mp_desc, last_octave, last_angle, Tcw, fx, fy, cx, cy, scale_factors, th, Tlw, bf, mb, False, train_blocked)
        wp = np.ascontiguousarray(world_pos, np.float32); va = np.ascontiguousarray(valid, np.uint8); bl = np.ascontiguousarray(blocks, np.uint8)
        md = np.ascontiguousarray(mp_desc, np.uint8); lo = np.ascontiguousarray(last_octave, np.int32); la = np.ascontiguousarray(last_angle, np.float32)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1)[:12].copy(); sf = np.ascontiguousarray(scale_factors, np.float32)
        tm = np.zeros(max(self.N, 1), np.int32); n = C.c_int()
        check(self.ctx.ptr, lib().cs_match_by_projection_frame(self.ctx.ptr, self._m, len(va), ptr(wp), ptr(va), ptr(bl), ptr(md), ptr(lo), ptr(la), ptr(T), fx,
                                                               fy, cx, cy, ptr(sf), len(sf), th,
                                                               int(self.mbCheckOrientation), None if train_blocked is None else ptr(np.ascontiguousarray(train_blocked, np.uint8)),
                                                               ptr(tm), C.byref(n)), "cs_match_by_projection_frame")
        return tm[:self.N].copy(), n.value

    def SearchByProjectionFrameStereo(self, world_pos, valid, blocks, mp_desc, last_octave, last_angle, Tcw, fx, fy, cx, cy, scale_factors, th, Tlw, bf, mb, bMono=False, train_blocked=None):
        """cs_match_by_projection_frame_stereo with its own argument order: the search with LastFrame's pose, mbf, the baseline and bMono as the reference passes it (bMono=True needs
        neither Tlw nor set_u_right and gives the monocular search's bytes).  (train_match, nmatches); the direction is left in last_direction."""
        mono = int(bool(bMono))
        wp = np.ascontiguousarray(world_pos, np.float32); va = np.ascontiguousarray(valid, np.uint8); bl = np.ascontiguousarray(blocks, np.uint8)
        md = np.ascontiguousarray(mp_desc, np.uint8); lo = np.ascontiguousarray(last_octave, np.int32); la = np.ascontiguousarray(last_angle, np.float32)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(-1)[:12].copy(); sf = np.ascontiguousarray(scale_factors, np.float32)
        Tl = None if Tlw is None else np.ascontiguousarray(Tlw, np.float32).reshape(-1)[:12].copy()
        tb = None if train_blocked is None else np.ascontiguousarray(train_blocked, np.uint8)
        tm = np.zeros(max(self.N, 1), np.int32); n = C.c_int(); d = C.c_int()
        check(self.ctx.ptr, lib().cs_match_by_projection_frame_stereo(self.ctx.ptr, self._m, len(va), ptr(wp), ptr(va), ptr(bl), ptr(md), ptr(lo), ptr(la), ptr(T), fx, fy, cx, cy, ptr(sf),
                                                                      len(sf), th, int(self.mbCheckOrientation), ptr(tb), ptr(tm), C.byref(n), ptr(Tl), bf, mb, int(mono), C.byref(d)),
              "cs_match_by_projection_frame_stereo")
        self.last_direction = d.value
        return tm[:self.N].copy(), n.value

    def SearchByProjectionLocalMap(self, proj_xy, view_cos, pred_level, in_view, blocks, mp_desc, scale_factors, th, train_blocked=None, proj_xr=None):
        """ORBmatcher::SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:50-142) over the fields isInFrustum left: (train_match, nmatches).  proj_xr (mTrackProjXR per map
        point): the search applies the mvuRight test of :104-109 against the mvuRight given to set_u_right."""
        if proj_xr is not None:
            return self._search_local_map_stereo(proj_xy, view_cos, pred_level, in_view, blocks, mp_desc, scale_factors, th, train_blocked, proj_xr)
        pxy = np.ascontiguousarray(proj_xy, np.float32); vc = np.ascontiguousarray(view_cos, np.float32); pl = np.ascontiguousarray(pred_level, np.int32)
        iv = np.ascontiguousarray(in_view, np.uint8); bl = np.ascontiguousarray(blocks, np.uint8); md = np.ascontiguousarray(mp_desc, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        tb = None if train_blocked is None else np.ascontiguousarray(train_blocked, np.uint8)
        tm = np.zeros(max(self.N, 1), np.int32); n = C.c_int()
        check(self.ctx.ptr, lib().cs_match_local_map(self.ctx.ptr, self._m, len(iv), ptr(pxy), ptr(vc), ptr(pl), ptr(iv),
                                                     ptr(bl), ptr(md), ptr(sf), len(sf), th, self.mfNNratio, ptr(tb), ptr(tm), C.byref(n)), "cs_match_local_map")
        return tm[:self.N].copy(), n.value

    def _search_local_map_stereo(self, proj_xy, view_cos, pred_level, in_view, blocks, mp_desc, scale_factors, th, train_blocked, proj_xr):
        pxy = np.ascontiguousarray(proj_xy, np.float32); vc = np.ascontiguousarray(view_cos, np.float32); pl = np.ascontiguousarray(pred_level, np.int32)
        iv = np.ascontiguousarray(in_view, np.uint8); bl = np.ascontiguousarray(blocks, np.uint8); md = np.ascontiguousarray(mp_desc, np.uint8)
        sf = np.ascontiguousarray(scale_factors, np.float32); xr = np.ascontiguousarray(proj_xr, np.float32)
        assert len(xr) == len(iv)
        tb = None if train_blocked is None else np.ascontiguousarray(train_blocked, np.uint8)
        tm = np.zeros(max(self.N, 1), np.int32); n = C.c_int()
        check(self.ctx.ptr, lib().cs_match_local_map_stereo(self.ctx.ptr, self._m, len(iv), ptr(pxy), ptr(vc), ptr(pl), ptr(iv), ptr(bl), ptr(md), ptr(sf), len(sf), th, self.mfNNratio,
                                                            ptr(tb), ptr(tm), C.byref(n), ptr(xr if len(xr) else np.zeros(1, np.float32))), "cs_match_local_map_stereo")
        return tm[:self.N].copy(), n.value

    def SearchForInitialization(self, keys1Un, desc1, vbPrevMatched, windowSize=100):
        k1 = np.ascontiguousarray(keys1Un, KEYPOINT_DTYPE); d1 = np.ascontiguousarray(desc1, np.uint8)
        prev = np.ascontiguousarray(vbPrevMatched, np.float32).copy()
        m12 = np.zeros(max(len(k1), 1), np.int32); n = C.c_int()
        check(self.ctx.ptr, lib().cs_match_for_initialization(self.ctx.ptr, self._m, ptr(k1), ptr(d1), len(k1), ptr(prev),
                                                              int(windowSize), self.mfNNratio, int(self.mbCheckOrientation), ptr(m12),
                                                              C.byref(n)), "cs_match_for_initialization")
        return m12[:len(k1)].copy(), prev, n.value

    def Fuse(self, u_right, inv_level_sigma2, uv, ur, pred_level, valid, mp_desc, scale_factors, th=3.0, keys_static=None):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th), the search (ORBmatcher.cc:921-983) against the key frame given to set_frame: per map
        point (bestIdx, bestDist); the third value is nFused."""
        uvv = np.ascontiguousarray(uv, np.float32); urr = np.ascontiguousarray(ur, np.float32); pl = np.ascontiguousarray(pred_level, np.int32)
        va = np.ascontiguousarray(valid, np.uint8); md = np.ascontiguousarray(mp_desc, np.uint8); sf = np.ascontiguousarray(scale_factors, np.float32)
        kr = np.ascontiguousarray(u_right, np.float32); isg = np.ascontiguousarray(inv_level_sigma2, np.float32)
        ks = None if keys_static is None else np.ascontiguousarray(keys_static, np.uint8)
        bi = np.zeros(max(len(va), 1), np.int32); bd = np.zeros(max(len(va), 1), np.int32); n = C.c_int()
        check(self.ctx.ptr, lib().cs_match_fuse(self.ctx.ptr, self._m, ptr(kr), ptr(isg), len(isg), ptr(ks), len(va),
                                                ptr(uvv), ptr(urr), ptr(pl), ptr(va), ptr(md), ptr(sf), th, ptr(bi), ptr(bd), C.byref(n)), "cs_match_fuse")
        return bi[:len(va)].copy(), bd[:len(va)].copy(), n.value

    @staticmethod
    def _map_points(world_pos, min_distance, max_distance, skip, mp_desc, normal=None):
        a = [np.ascontiguousarray(world_pos, np.float32), np.ascontiguousarray(min_distance, np.float32), np.ascontiguousarray(max_distance, np.float32),
             np.ascontiguousarray(skip, np.uint8), np.ascontiguousarray(mp_desc, np.uint8)]
        if normal is not None:
            a.append(np.ascontiguousarray(normal, np.float32))
        return a

    @staticmethod
    def _f(a, n):
        a = np.ascontiguousarray(a, np.float32).reshape(-1)
        assert a.size == n
        return a

    def SearchByProjectionReloc(self, Rcw, tcw, Ow, world_pos, min_distance, max_distance, skip, kf_angle, mp_desc, fx, fy, cx, cy, log_scale_factor, scale_factors, th, ORBdist, train_blocked=None):
        """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:1727-1858) against the current frame given to set_frame: (train_match per
        key point of the current frame = index of pKF's map point or -1, nmatches, points dropped because their predicted level is outside the scale table)."""
        wp, mn, mx, sk, md = self._map_points(world_pos, min_distance, max_distance, skip, mp_desc)
        R, t, O = self._f(Rcw, 9), self._f(tcw, 3), self._f(Ow, 3); ka = np.ascontiguousarray(kf_angle, np.float32); sf = np.ascontiguousarray(scale_factors, np.float32)
        tb = None if train_blocked is None else np.ascontiguousarray(train_blocked, np.uint8)
        tm = np.zeros(max(self.N, 1), np.int32); n = C.c_int(); no = C.c_int()
        check(self.ctx.ptr, lib().cs_match_by_projection_reloc(self.ctx.ptr, self._m, ptr(R), ptr(t), ptr(O), len(sk), ptr(wp), ptr(mn),
                                                               ptr(mx), ptr(sk), ptr(ka), ptr(md), ptr(tb), fx, fy, cx, cy, log_scale_factor, ptr(sf), len(sf),
                                                               th, int(ORBdist), int(self.mbCheckOrientation), ptr(tm), C.byref(n), C.byref(no)),
              "cs_match_by_projection_reloc")
        return tm[:self.N].copy(), n.value, no.value

    def SearchByProjectionSim3(self, Rcw, tcw, Ow, world_pos, normal, min_distance, max_distance, skip, mp_desc, fx, fy, cx, cy, log_scale_factor, scale_factors, th, train_blocked=None):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (ORBmatcher.cc:309-427) against the key frame given to set_frame: (train_match per key point = index
        into vpPoints or -1, nmatches, points outside the scale table).  train_blocked = vpMatched[idx] != NULL or not KeysStatic[idx]."""
        wp, mn, mx, sk, md, nr = self._map_points(world_pos, min_distance, max_distance, skip, mp_desc, normal)
        R, t, O = self._f(Rcw, 9), self._f(tcw, 3), self._f(Ow, 3); sf = np.ascontiguousarray(scale_factors, np.float32)
        tb = None if train_blocked is None else np.ascontiguousarray(train_blocked, np.uint8)
        tm = np.zeros(max(self.N, 1), np.int32); n = C.c_int(); no = C.c_int()
        check(self.ctx.ptr, lib().cs_match_by_projection_sim3(self.ctx.ptr, self._m, ptr(R), ptr(t), ptr(O), len(sk), ptr(wp), ptr(nr),
                                                              ptr(mn), ptr(mx), ptr(sk), ptr(md), ptr(tb), fx, fy, cx, cy, log_scale_factor, ptr(sf), len(sf),
                                                              th, ptr(tm), C.byref(n), C.byref(no)), "cs_match_by_projection_sim3")
        return tm[:self.N].copy(), n.value, no.value

    def FuseSim3(self, Rcw, tcw, Ow, world_pos, normal, min_distance, max_distance, skip, mp_desc, fx, fy, cx, cy, log_scale_factor, scale_factors, th, train_blocked=None):
        """ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint), the search (ORBmatcher.cc:1033-1118), against the key frame given to set_frame: (best_idx, best_dist per map
        point, nFused, points outside the scale table).  train_blocked = not KeysStatic[idx]."""
        wp, mn, mx, sk, md, nr = self._map_points(world_pos, min_distance, max_distance, skip, mp_desc, normal)
        R, t, O = self._f(Rcw, 9), self._f(tcw, 3), self._f(Ow, 3); sf = np.ascontiguousarray(scale_factors, np.float32)
        tb = None if train_blocked is None else np.ascontiguousarray(train_blocked, np.uint8)
        bi = np.zeros(max(len(sk), 1), np.int32); bd = np.zeros(max(len(sk), 1), np.int32); n = C.c_int(); no = C.c_int()
        check(self.ctx.ptr, lib().cs_match_fuse_sim3(self.ctx.ptr, self._m, ptr(R), ptr(t), ptr(O), len(sk), ptr(wp), ptr(nr),
                                                     ptr(mn), ptr(mx), ptr(sk), ptr(md), ptr(tb), fx, fy, cx, cy, log_scale_factor, ptr(sf), len(sf),
                                                     th, ptr(bi), ptr(bd), C.byref(n), C.byref(no)), "cs_match_fuse_sim3")
        return bi[:len(sk)].copy(), bd[:len(sk)].copy(), n.value, no.value

    def SearchLocalPoints(self, Rcw, tcw, Ow, world_pos, normal, min_distance, max_distance, skip, blocks, mp_desc, fx, fy, cx, cy, bf, log_scale_factor, scale_factors, th,
                          viewing_cos_limit=0.5, train_blocked=None, stereo=False):
        """Tracking::SearchLocalPoints (Tracking.cc:2696-2727): Frame::isInFrustum per local map point and ORBmatcher::SearchByProjection(F, vpMapPoints, th) against the current
        frame given to set_frame, in one call.  stereo: with the mvuRight test of ORBmatcher.cc:104-109 against the mvuRight given to set_u_right.  Returns a dict: train_match per key point (index of the local point or -1), nmatches, n_to_match, outside (points dropped because
        their predicted level is outside the scale table) and, per local point, in_view, proj (u, v, uR), pred_level, view_cos."""
        wp, mn, mx, sk, md, nr = self._map_points(world_pos, min_distance, max_distance, skip, mp_desc, normal)
        R, t, O = self._f(Rcw, 9), self._f(tcw, 3), self._f(Ow, 3); sf = np.ascontiguousarray(scale_factors, np.float32); bl = np.ascontiguousarray(blocks, np.uint8)
        tb = None if train_blocked is None else np.ascontiguousarray(train_blocked, np.uint8)
        n_mp = len(sk); k = max(n_mp, 1)
        tm = np.zeros(max(self.N, 1), np.int32); n = C.c_int(); nt = C.c_int(); no = C.c_int()
        iv = np.zeros(k, np.uint8); pj = np.zeros((k, 3), np.float32); pl = np.full(k, -1, np.int32); vc = np.zeros(k, np.float32)
        entry = "cs_match_local_map_frustum_stereo" if stereo else "cs_match_local_map_frustum"
        check(self.ctx.ptr, getattr(lib(), entry)(self.ctx.ptr, self._m, ptr(R), ptr(t), ptr(O), n_mp, ptr(wp), ptr(nr),
                                                             ptr(mn), ptr(mx), ptr(sk), ptr(bl), ptr(md), ptr(tb), fx, fy, cx, cy, bf,
                                                             log_scale_factor, ptr(sf), len(sf), viewing_cos_limit, th, self.mfNNratio,
                                                             ptr(tm), C.byref(n), C.byref(nt), C.byref(no), ptr(iv), ptr(pj), ptr(pl), ptr(vc)),
              entry)
        return {"train_match": tm[:self.N].copy(), "nmatches": n.value, "n_to_match": nt.value, "outside": no.value, "in_view": iv[:n_mp], "proj": pj[:n_mp], "pred_level": pl[:n_mp],
                "view_cos": vc[:n_mp]}

    def FuseMap(self, u_right, inv_level_sigma2, Rcw, tcw, Ow, world_pos, normal, min_distance, max_distance, skip, mp_desc, fx, fy, cx, cy, bf, log_scale_factor, scale_factors, th=3.0,
                keys_static=None):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) with its preamble (ORBmatcher.cc:871-983) against the key frame given to set_frame: (best_idx, best_dist per map point, nFused,
        points outside the scale table)."""
        wp, mn, mx, sk, md, nr = self._map_points(world_pos, min_distance, max_distance, skip, mp_desc, normal)
        R, t, O = self._f(Rcw, 9), self._f(tcw, 3), self._f(Ow, 3); sf = np.ascontiguousarray(scale_factors, np.float32)
        kr = np.ascontiguousarray(u_right, np.float32); isg = np.ascontiguousarray(inv_level_sigma2, np.float32)
        assert len(isg) == len(sf)
        ks = None if keys_static is None else np.ascontiguousarray(keys_static, np.uint8)
        bi = np.zeros(max(len(sk), 1), np.int32); bd = np.zeros(max(len(sk), 1), np.int32); n = C.c_int(); no = C.c_int()
        check(self.ctx.ptr, lib().cs_match_fuse_map(self.ctx.ptr, self._m, ptr(kr), ptr(isg), len(isg), ptr(ks), ptr(R),
                                                    ptr(t), ptr(O), len(sk), ptr(wp), ptr(nr), ptr(mn), ptr(mx), ptr(sk),
                                                    ptr(md), fx, fy, cx, cy, bf, log_scale_factor, ptr(sf),
                                                    th, ptr(bi), ptr(bd), C.byref(n), C.byref(no)), "cs_match_fuse_map")
        return bi[:len(sk)].copy(), bd[:len(sk)].copy(), n.value, no.value

    def SearchBySim3(self, other, R1w, t1w, R2w, t2w, sR12, t12, sR21, t21, points1, points2, fx, fy, cx, cy, log_scale_factor, scale_factors, th, train_blocked1=None, train_blocked2=None):
        """ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (ORBmatcher.cc:1141-1371); self holds KF1, `other` KF2.  points_k = (world_pos, min_distance,
        max_distance, skip, mp_desc) of KFk's map points, one per key point.  Returns (matches12 per key point of KF1 = key point of KF2 or -1, nFound, points outside the scale table)."""
        a1 = self._map_points(*points1); a2 = self._map_points(*points2)
        Ts = [self._f(x, k) for x, k in ((R1w, 9), (t1w, 3), (R2w, 9), (t2w, 3), (sR12, 9), (t12, 3), (sR21, 9), (t21, 3))]
        sf = np.ascontiguousarray(scale_factors, np.float32)
        tb1 = None if train_blocked1 is None else np.ascontiguousarray(train_blocked1, np.uint8); tb2 = None if train_blocked2 is None else np.ascontiguousarray(train_blocked2, np.uint8)
        side = lambda a, tb: (len(a[3]), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(a[4]), ptr(tb))
        m12 = np.zeros(max(len(a1[3]), 1), np.int32); n = C.c_int(); no = C.c_int()
        check(self.ctx.ptr, lib().cs_match_by_sim3(self.ctx.ptr, self._m, other._m, *[ptr(x) for x in Ts], *side(a1, tb1), *side(a2, tb2), fx, fy, cx,
                                                   cy, log_scale_factor, ptr(sf), len(sf), th, ptr(m12), C.byref(n), C.byref(no)),
              "cs_match_by_sim3")
        return m12[:len(a1[3])].copy(), n.value, no.value

    def SearchForTriangulation(self, keys1Un, desc1, node1, skip1, ur1, keys2Un, desc2, node2, skip2, ur2, F12, ex, ey, scale_factors2, level_sigma2_2, bOnlyStereo=False):
        """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo) (ORBmatcher.cc:679-850): matches12 and nmatches."""
        k1 = np.ascontiguousarray(keys1Un, KEYPOINT_DTYPE); d1 = np.ascontiguousarray(desc1, np.uint8); k2 = np.ascontiguousarray(keys2Un, KEYPOINT_DTYPE)
        d2 = np.ascontiguousarray(desc2, np.uint8)
        n1 = np.ascontiguousarray(node1, np.int32); s1 = np.ascontiguousarray(skip1, np.uint8); u1 = np.ascontiguousarray(ur1, np.float32)
        n2 = np.ascontiguousarray(node2, np.int32); s2 = np.ascontiguousarray(skip2, np.uint8); u2 = np.ascontiguousarray(ur2, np.float32)
        Fm = np.ascontiguousarray(F12, np.float32).reshape(-1); sf = np.ascontiguousarray(scale_factors2, np.float32); sg = np.ascontiguousarray(level_sigma2_2, np.float32)
        m12 = np.zeros(max(len(k1), 1), np.int32); n = C.c_int()
        check(self.ctx.ptr, lib().cs_match_for_triangulation(self.ctx.ptr, ptr(k1), ptr(d1), len(k1), ptr(n1), ptr(s1),
                                                             ptr(u1), ptr(k2), ptr(d2), len(k2), ptr(n2), ptr(s2), ptr(u2), ptr(Fm), ex, ey, ptr(sf), ptr(sg), len(sf),
                                                             int(bOnlyStereo), int(self.mbCheckOrientation), ptr(m12), C.byref(n)), "cs_match_for_triangulation")
        return m12[:len(k1)].copy(), n.value

    def SearchByBoW(self, keysKF, descKF, nodeKF, skipKF, keysF, descF, nodeF, skipF=None):
        """ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) (ORBmatcher.cc:171-310): per frame feature the key-frame feature whose map
        point it receives (-1 none), and nmatches."""
        kk = np.ascontiguousarray(keysKF, KEYPOINT_DTYPE); dk = np.ascontiguousarray(descKF, np.uint8); kf = np.ascontiguousarray(keysF, KEYPOINT_DTYPE)
        df = np.ascontiguousarray(descF, np.uint8)
        nk = np.ascontiguousarray(nodeKF, np.int32); sk = np.ascontiguousarray(skipKF, np.uint8); nf = np.ascontiguousarray(nodeF, np.int32)
        sf = None if skipF is None else np.ascontiguousarray(skipF, np.uint8)
        mf = np.zeros(max(len(kf), 1), np.int32); n = C.c_int()
        check(self.ctx.ptr, lib().cs_match_by_bow(self.ctx.ptr, ptr(kk), ptr(dk), len(kk), ptr(nk), ptr(sk), ptr(kf), ptr(df), len(kf), ptr(nf), ptr(sf),
                                                  self.mfNNratio, int(self.mbCheckOrientation), ptr(mf), C.byref(n)), "cs_match_by_bow")
        return mf[:len(kf)].copy(), n.value

    def SearchByBoWKeyFrames(self, keys1, desc1, node1, skip1, keys2, desc2, node2, skip2):
        """ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (ORBmatcher.cc:544-677): per KF1 feature the KF2 feature whose map point it is matched
        to (-1 none), and nmatches.  skip = the feature has no usable map point."""
        k1 = np.ascontiguousarray(keys1, KEYPOINT_DTYPE); d1 = np.ascontiguousarray(desc1, np.uint8); k2 = np.ascontiguousarray(keys2, KEYPOINT_DTYPE)
        d2 = np.ascontiguousarray(desc2, np.uint8)
        n1 = np.ascontiguousarray(node1, np.int32); s1 = np.ascontiguousarray(skip1, np.uint8); n2 = np.ascontiguousarray(node2, np.int32)
        s2 = np.ascontiguousarray(skip2, np.uint8)
        m12 = np.zeros(max(len(k1), 1), np.int32); n = C.c_int()
        check(self.ctx.ptr, lib().cs_match_by_bow_kf(self.ctx.ptr, ptr(k1), ptr(d1), len(k1), ptr(n1), ptr(s1), ptr(k2), ptr(d2), len(k2), ptr(n2), ptr(s2),
                                                     self.mfNNratio, int(self.mbCheckOrientation), ptr(m12), C.byref(n)), "cs_match_by_bow_kf")
        return m12[:len(k1)].copy(), n.value


class ORBmatcherStream(Handle):
    """SearchByProjection(CurrentFrame, LastFrame) for a whole window of a stream that an ORBextractor holds in HBM (cs_match_by_projection_stream)."""
    HANDLE, DESTROY = "_m", "cs_match_stream_destroy"

    def __init__(self, mbCheckOrientation=True, ctx=None):
        self.ctx = ctx
        self.mbCheckOrientation = bool(mbCheckOrientation)
        self._m = C.c_void_p()
        check(ctx.ptr, lib().cs_match_stream_create(C.byref(self._m)), "cs_match_stream_create")

    def search(self, orb, f0, n_pairs, K4, dist5, bounds, world_pos, valid, blocks, Tcw, fx, fy, cx, cy, scale_factors, th, n_train, mp_desc=None, bMono=True, Tlw=None, u_right=None,
               bf=0.0, mb=0.0):
        """world_pos / valid / blocks: concatenated over the last frames f0 .. f0 + n_pairs - 1; Tcw: (n_pairs, 3, 4); n_train: key points of frames f0 + 1 .. f0 + n_pairs.
        Returns (train_match concatenated over the current frames, nmatches per pair).  bMono=False: the stereo branch (cs_match_by_projection_stream_stereo) -- Tlw (n_pairs, 3, 4)
        the last frames' poses, u_right = mvuRight packed over the current frames (n_train floats, or a device address), bf, mb; the directions are left in last_direction."""
        if not bMono:
            return self.search_stereo(orb, f0, n_pairs, K4, dist5, bounds, world_pos, valid, blocks, Tcw, fx, fy, cx, cy, scale_factors, th, n_train, Tlw, u_right, bf, mb, False, mp_desc)
        k4 = np.ascontiguousarray(K4, np.float32); d5 = None if dist5 is None else np.ascontiguousarray(dist5, np.float32)
        wp = np.ascontiguousarray(world_pos, np.float32); va = np.ascontiguousarray(valid, np.uint8); bl = np.ascontiguousarray(blocks, np.uint8)
        T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(n_pairs, -1)[:, :12]); sf = np.ascontiguousarray(scale_factors, np.float32)
        md = None if mp_desc is None else np.ascontiguousarray(mp_desc, np.uint8)
        tm = np.zeros(max(int(n_train), 1), np.int32); nm = np.zeros(n_pairs, np.int32)
        check(self.ctx.ptr, lib().cs_match_by_projection_stream(self.ctx.ptr, self._m, orb._e, int(f0), int(n_pairs), ptr(k4), ptr(d5),
                                                                bounds[0], bounds[1], bounds[2], bounds[3], len(va), int(n_train), ptr(wp), ptr(va),
                                                                ptr(bl), ptr(md), ptr(T), fx, fy, cx,
                                                                cy, ptr(sf), len(sf), th, int(self.mbCheckOrientation), ptr(tm), ptr(nm)),
              "cs_match_by_projection_stream")
        return tm[:int(n_train)], nm

    def search_stereo(self, orb, f0, n_pairs, K4, dist5, bounds, world_pos, valid, blocks, Tcw, fx, fy, cx, cy, scale_factors, th, n_train, Tlw, u_right, bf, mb, bMono=False, mp_desc=None):
        """cs_match_by_projection_stream_stereo with its own argument order (bMono=True needs neither Tlw nor u_right and gives the monocular window search's bytes)."""
        mono = int(bool(bMono))
        k4 = np.ascontiguousarray(K4, np.float32); d5 = None if dist5 is None else np.ascontiguousarray(dist5, np.float32)
        wp = np.ascontiguousarray(world_pos, np.float32); va = np.ascontiguousarray(valid, np.uint8); bl = np.ascontiguousarray(blocks, np.uint8)
        T = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(n_pairs, -1)[:, :12]); sf = np.ascontiguousarray(scale_factors, np.float32)
        Tl = None if Tlw is None else np.ascontiguousarray(np.asarray(Tlw, np.float32).reshape(n_pairs, -1)[:, :12])
        md = None if mp_desc is None else np.ascontiguousarray(mp_desc, np.uint8)
        on_device = isinstance(u_right, (int, np.integer))
        if on_device:
            ur = C.cast(C.c_void_p(int(u_right)), C.POINTER(C.c_float))
        else:
            ur_a = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
            assert ur_a is None or len(ur_a) == int(n_train)
            ur = ptr(ur_a)
        tm = np.zeros(max(int(n_train), 1), np.int32); nm = np.zeros(n_pairs, np.int32); dr = np.zeros(n_pairs, np.int32)
        check(self.ctx.ptr, lib().cs_match_by_projection_stream_stereo(self.ctx.ptr, self._m, orb._e, int(f0), int(n_pairs), ptr(k4), ptr(d5), bounds[0], bounds[1], bounds[2], bounds[3],
                                                                       len(va), int(n_train), ptr(wp), ptr(va), ptr(bl), ptr(md), ptr(T), fx, fy, cx, cy, ptr(sf), len(sf), th,
                                                                       int(self.mbCheckOrientation), ptr(tm), ptr(nm), ptr(Tl), ur, int(on_device), bf, mb, int(mono), ptr(dr)),
              "cs_match_by_projection_stream_stereo")
        self.last_direction = dr
        return tm[:int(n_train)], nm

    def last_counts(self):
        q, c = C.c_long(), C.c_long()
        check(self.ctx.ptr, lib().cs_match_stream_last_counts(self._m, C.byref(q), C.byref(c)), "cs_match_stream_last_counts")
        return {"queries": q.value, "candidates": c.value}


def hamming_knn2(ctx, q, t):
    q = np.ascontiguousarray(q, np.uint8); t = np.ascontiguousarray(t, np.uint8)
    bi = np.zeros(max(len(q), 1), np.int32); bd = np.zeros(max(len(q), 1), np.int32); sd = np.zeros(max(len(q), 1), np.int32)
    check(ctx.ptr, lib().cs_hamming_knn2(ctx.ptr, ptr(q), len(q), ptr(t), len(t), ptr(bi), ptr(bd), ptr(sd)), "cs_hamming_knn2")
    return bi[:len(q)], bd[:len(q)], sd[:len(q)]


def frame_image_bounds(cols, rows, K4, dist5=None):
    """Frame::ComputeImageBounds -> (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    k4 = np.ascontiguousarray(K4, np.float32)
    d5 = None if dist5 is None else np.ascontiguousarray(dist5, np.float32)
    b = np.zeros(4, np.float32)
    r = lib().cs_frame_image_bounds(int(cols), int(rows), ptr(k4), ptr(d5), ptr(b))
    if r != 0:
        raise RuntimeError("cs_frame_image_bounds failed: %d" % r)
    return b
