"""Python host-side mirror of the middle of ORB_SLAM2::LocalMapping's key-frame cycle (reference orb_object_slam/src/LocalMapping.cc:319-570, MapPoint.cc:381-446, :469-510):
CreateNewMapPoints' neighbour loop over cs_match_for_triangulation and cs_create_new_map_points, and MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth for many
points per call."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, lib, ptr
from .orb import KEYPOINT_DTYPE

MAX_NEIGHBOURS = 32
STATUS = ("created", "parallax", "w_zero", "z1", "z2", "reproj1", "reproj2", "zero_dist", "scale", "claimed", "stereo_no_depth")


class CsLmFrame(C.Structure):
    """cs_lm_frame of include/cubeslam_hip.h."""
    _fields_ = [("keysUn", C.c_void_p), ("keys_xy", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p), ("N", C.c_int), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3),
                ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float), ("mbf", C.c_float),
                ("mb", C.c_float), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("n_levels", C.c_int), ("scale_factor", C.c_float)]


class KeyFrameView:
    """What CreateNewMapPoints reads of a KeyFrame, as flat arrays: mvKeysUn, mvKeys' points, mvuRight, mvDepth, GetRotation / GetTranslation / GetCameraCenter as stored, the
    intrinsics, mvScaleFactors, mvLevelSigma2, mfScaleFactor; for the search also mDescriptors, the vocabulary node of every feature (cs_bow_transform) and skip[i] = the key
    point has a map point or is not static."""

    def __init__(self, keysUn, keys_xy, u_right, depth, Rcw, tcw, Ow, fx, fy, cx, cy, invfx, invfy, mbf, mb, scale_factors, level_sigma2, scale_factor, desc=None, node=None,
                 skip=None):
        f32 = lambda a, n=None: np.ascontiguousarray(a, np.float32).reshape(-1 if n is None else n)
        self.keysUn = np.ascontiguousarray(keysUn, KEYPOINT_DTYPE)
        self.N = len(self.keysUn)
        self.keys_xy, self.u_right, self.depth = f32(keys_xy, 2 * self.N), f32(u_right, self.N), f32(depth, self.N)
        self.Rcw, self.tcw, self.Ow = f32(Rcw, 9), f32(tcw, 3), f32(Ow, 3)
        self.fx, self.fy, self.cx, self.cy, self.invfx, self.invfy, self.mbf, self.mb = (np.float32(v) for v in (fx, fy, cx, cy, invfx, invfy, mbf, mb))
        self.scale_factors, self.level_sigma2 = f32(scale_factors), f32(level_sigma2)
        if len(self.scale_factors) != len(self.level_sigma2):
            raise ValueError("mvScaleFactors and mvLevelSigma2 differ in length")
        self.scale_factor = np.float32(scale_factor)
        self.desc = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(self.N, 32)
        self.node = None if node is None else np.ascontiguousarray(node, np.int32)
        self.skip = np.zeros(self.N, np.uint8) if skip is None else np.ascontiguousarray(skip, np.uint8)

    def c_struct(self):
        return CsLmFrame(self.keysUn.ctypes.data, self.keys_xy.ctypes.data, self.u_right.ctypes.data, self.depth.ctypes.data, self.N, (C.c_float * 9)(*self.Rcw),
                         (C.c_float * 3)(*self.tcw), (C.c_float * 3)(*self.Ow), self.fx, self.fy, self.cx, self.cy, self.invfx, self.invfy, self.mbf, self.mb,
                         self.scale_factors.ctypes.data, self.level_sigma2.ctypes.data, len(self.scale_factors), self.scale_factor)


def create_new_map_points(ctx, kf, neighbours, matches12):
    """cs_create_new_map_points: kf / neighbours are KeyFrameViews, matches12 (n_neigh, N1) the searches made with the initial skip1.  Returns pair_off, idx1, idx2, x3D, status,
    new_pair_of_idx1, nnew."""
    n = len(neighbours)
    m = np.ascontiguousarray(matches12, np.int32).reshape(n, kf.N)
    cap = int((m != -1).sum())  # (entries below -1 are the library's to refuse)
    off = np.zeros(n + 1, np.int32); i1 = np.zeros(max(cap, 1), np.int32); i2 = np.zeros(max(cap, 1), np.int32); x = np.zeros((max(cap, 1), 3), np.float32)
    st = np.zeros(max(cap, 1), np.uint8); new = np.zeros(max(kf.N, 1), np.int32); nnew = C.c_int()
    arr = (CsLmFrame * max(n, 1))(*[f.c_struct() for f in neighbours])
    cur = kf.c_struct()
    check(ctx.ptr, lib().cs_create_new_map_points(ctx.ptr, C.byref(cur), arr, n, ptr(m), cap, ptr(off), ptr(i1), ptr(i2), ptr(x),
                                                  ptr(st), ptr(new), C.byref(nnew)), "cs_create_new_map_points")
    return {"pair_off": off, "idx1": i1[:cap], "idx2": i2[:cap], "x3D": x[:cap], "status": st[:cap], "new_pair_of_idx1": new[:kf.N], "nnew": nnew.value}


class LocalMapping:
    def __init__(self, ctx=None, device=0, monocular=False, matcher=None):
        self.ctx = ctx or _lib.Context(device)
        self.mbMonocular = monocular
        self._matcher = matcher

    def _search(self, kf, nb, F12, epipole):
        """ORBmatcher(0.6, false).SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, vMatchedIndices, false) -> matches12."""
        if self._matcher is None:
            from .matcher import ORBmatcher
            self._matcher = ORBmatcher(0.6, False, ctx=self.ctx)
        m12, _ = self._matcher.SearchForTriangulation(kf.keysUn, kf.desc, kf.node, kf.skip, kf.u_right, nb.keysUn, nb.desc, nb.node, nb.skip, nb.u_right, F12, epipole[0],
                                                      epipole[1], nb.scale_factors, nb.level_sigma2, False)
        return m12

    def baseline_ok(self, kf, nb, median_depth=None):
        """:356-372: the baseline against the neighbour's mb (stereo / RGB-D) or against its scene's median depth, ComputeSceneMedianDepth(2), which the caller supplies."""
        d = [np.float32(nb.Ow[k]) - np.float32(kf.Ow[k]) for k in range(3)]
        baseline = np.float32(math.sqrt(sum(float(c) * float(c) for c in d)))
        if not self.mbMonocular:
            return not baseline < nb.mb
        if median_depth is None:
            raise ValueError("monocular: CreateNewMapPoints needs median_depths, one ComputeSceneMedianDepth(2) per neighbour")
        return not float(baseline / np.float32(median_depth)) < 0.01

    def CreateNewMapPoints(self, kf, neighbours, F12s, epipoles, median_depths=None, search=None):
        """The neighbour loop of LocalMapping::CreateNewMapPoints: neighbours = GetBestCovisibilityKeyFrames(nn) in order, F12s[i] = ComputeF12(kf, neighbours[i]), epipoles[i] the
        projection of kf's centre into neighbours[i] (ORBmatcher.cc:686-692), median_depths[i] = neighbours[i]->ComputeSceneMedianDepth(2) (monocular only).  One search per
        neighbour that passes the baseline test, with the initial skip of kf, then one cs_create_new_map_points.  search(kf, nb, F12, epipole) -> matches12 replaces the matcher.

        Returns the new points in the reference's creation order -- neighbour (its index in `neighbours`), idx1, idx2, x3D -- and every pair with its status.  A caller that
        honours CheckNewKeyFrames() (:351) and breaks off before neighbour i keeps the points with neighbour < i (points_before): a neighbour's pairs depend on earlier
        neighbours only, so those results are final."""
        if len(neighbours) > MAX_NEIGHBOURS:
            raise ValueError("more than %d neighbours" % MAX_NEIGHBOURS)
        search = search or self._search
        kept = [i for i, nb in enumerate(neighbours) if self.baseline_ok(kf, nb, None if median_depths is None else median_depths[i])]
        m = np.full((len(kept), kf.N), -1, np.int32)
        for r, i in enumerate(kept):
            m[r] = search(kf, neighbours[i], F12s[i], epipoles[i])
        out = create_new_map_points(self.ctx, kf, [neighbours[i] for i in kept], m)
        pair_neigh = np.repeat(np.asarray(kept, np.int32), np.diff(out["pair_off"]))
        created = np.sort(out["new_pair_of_idx1"][out["new_pair_of_idx1"] >= 0])  # pair order = creation order
        out.update(kept=kept, pair_neighbour=pair_neigh, new_neighbour=pair_neigh[created], new_idx1=out["idx1"][created], new_idx2=out["idx2"][created],
                   new_x3D=out["x3D"][created])
        return out

    @staticmethod
    def points_before(result, i):
        """The new points a reference that returns at `i > 0 && CheckNewKeyFrames()` before neighbour i has created."""
        k = result["new_neighbour"] < i
        return result["new_neighbour"][k], result["new_idx1"][k], result["new_idx2"][k], result["new_x3D"][k]


def ComputeDistinctiveDescriptors(ctx, obs_off, desc):
    """MapPoint::ComputeDistinctiveDescriptors for many points: obs_off[n + 1] (CSR), desc = the observations' descriptors in the iteration order of mObservations with bad key
    frames left out.  best[n]: index within the run of the descriptor that becomes mDescriptor, -1 for an empty run."""
    off = np.ascontiguousarray(obs_off, np.int32); d = np.ascontiguousarray(desc, np.uint8)
    n = len(off) - 1
    best = np.zeros(max(n, 1), np.int32)
    check(ctx.ptr, lib().cs_mappoint_distinctive_descriptors(ctx.ptr, n, ptr(off), ptr(d), ptr(best)), "cs_mappoint_distinctive_descriptors")
    return best[:n]


def UpdateNormalAndDepth(ctx, world_pos, obs_off, obs_kf, kf_Ow, ref_kf, ref_octave, scale_factors, normal=None, min_distance=None, max_distance=None):
    """MapPoint::UpdateNormalAndDepth for many points.  normal / min_distance / max_distance: the current values, kept for points without observations (zeros when not given).
    Returns (mNormalVector, mfMinDistance, mfMaxDistance, updated)."""
    pos = np.ascontiguousarray(world_pos, np.float32).reshape(-1, 3); n = len(pos)
    off = np.ascontiguousarray(obs_off, np.int32); ob = np.ascontiguousarray(obs_kf, np.int32); ow = np.ascontiguousarray(kf_Ow, np.float32).reshape(-1, 3)
    rk = np.ascontiguousarray(ref_kf, np.int32); ro = np.ascontiguousarray(ref_octave, np.int32); sf = np.ascontiguousarray(scale_factors, np.float32)
    if len(off) != n + 1 or len(rk) != n or len(ro) != n:
        raise ValueError("obs_off, ref_kf and ref_octave must have one entry per point (obs_off one more)")
    nv = np.zeros((max(n, 1), 3), np.float32) if normal is None else np.array(normal, np.float32).reshape(-1, 3)
    mn = np.zeros(max(n, 1), np.float32) if min_distance is None else np.array(min_distance, np.float32)
    mx = np.zeros(max(n, 1), np.float32) if max_distance is None else np.array(max_distance, np.float32)
    up = np.zeros(max(n, 1), np.uint8)
    check(ctx.ptr, lib().cs_mappoint_update_normal_and_depth(ctx.ptr, n, ptr(pos), ptr(off), ptr(ob), len(ow), ptr(ow), ptr(rk),
                                                             ptr(ro), ptr(sf), len(sf), ptr(nv), ptr(mn), ptr(mx), ptr(up)),
          "cs_mappoint_update_normal_and_depth")
    return nv[:n], mn[:n], mx[:n], up[:n]
