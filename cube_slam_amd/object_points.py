"""Python host-side mirror of include/cubeslam_hip/object_points.h: the dynamic-point triangulation of Tracking::CreateNewKeyFrame (reference
orb_object_slam/src/Tracking.cc:2144-2244) and the object-depth initialisation (Tracking.cc:876-898, :2339-2424, LocalMapping.cc:574-652), many key frames per call.
ctx = None takes the library's host form (the same statements, no device)."""
import numpy as np

from ._lib import check, lib, ptr

TRIANGULATED, NO_OBSERVATION, TRACKLET, W_ZERO, TOO_FAR = range(5)  # status bytes of triangulate_dynamic_points
FIRST_FRAME, TRACKING, LOCAL_MAPPING = range(3)  # modes of object_depth_points
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])  # cs_keypoint


def _a(x, dtype, shape=(-1,)):
    return None if x is None else np.ascontiguousarray(x, dtype).reshape(shape)


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int32)
    off[1:] = np.cumsum(counts)
    return off


def triangulate_dynamic_points(ctx, first, Tcw_last, Tcw_now, K4, cub_first_last, cub_pose_last, cub_first_now, cub_pose_now, kp1, kp2, obj_last, obj_now, idx_last,
                               world_pos, tracklet_last=None, tracklet_now=None):
    """cs_triangulate_dynamic_points over flat arrays (see the header for each).  Returns a dict: status [P] uint8, x3D [P, 3] float32, pos_to_obj [P, 3] float32 and
    dpoints [P, 3] float64 (the layout cs_ba_dyn_problem reads)."""
    first = _a(first, np.int32)
    n_pairs = len(first) - 1
    P = int(first[-1]) if n_pairs > 0 else 0
    n = max(P, 1)
    out = {"status": np.zeros(n, np.uint8), "x3D": np.zeros((n, 3), np.float32), "pos_to_obj": np.zeros((n, 3), np.float32), "dpoints": np.zeros((n, 3), np.float64)}
    args = [_a(Tcw_last, np.float32), _a(Tcw_now, np.float32), _a(K4, np.float32), _a(cub_first_last, np.int32), _a(cub_pose_last, np.float64), _a(cub_first_now, np.int32),
            _a(cub_pose_now, np.float64), _a(tracklet_last, np.int32), _a(tracklet_now, np.int32), _a(kp1, np.float32), _a(kp2, np.float32), _a(obj_last, np.int32),
            _a(obj_now, np.int32), _a(idx_last, np.int32), _a(world_pos, np.float32)]
    c = ctx.ptr if ctx is not None else None
    r = lib().cs_triangulate_dynamic_points(c, n_pairs, ptr(first), *[ptr(a) for a in args], ptr(out["status"]), ptr(out["x3D"]), ptr(out["pos_to_obj"]), ptr(out["dpoints"]))
    check(c, r, "cs_triangulate_dynamic_points")
    return {k: v[:P] for k, v in out.items()}


def object_depth_points(ctx, mode, first, keys, has_map_point, object_id, cub_first, cuboid_depth, K4, Twc, bounds=None, draw_first=None, draws=None):
    """cs_object_depth_points over flat arrays (see the header for each).  keys: a KEYPOINT_DTYPE array.  Returns a dict: n_candidates, raw_depth_pts, max_initialize_pts
    [F]; cand_first [F + 1] with candidates and shuffled; new_first [F + 1] with new_idx and new_x3D [n, 3]."""
    first = _a(first, np.int32)
    F = len(first) - 1
    total = max(int(first[-1]) if F > 0 else 0, 1)
    keys = None if keys is None else np.ascontiguousarray(keys, KEYPOINT_DTYPE).reshape(-1)
    out = {"n_candidates": np.zeros(max(F, 1), np.int32), "raw_depth_pts": np.zeros(max(F, 1), np.int32), "max_initialize_pts": np.zeros(max(F, 1), np.int32),
           "cand_first": np.zeros(F + 1, np.int32), "candidates": np.zeros(total, np.int32), "shuffled": np.zeros(total, np.int32), "new_first": np.zeros(F + 1, np.int32),
           "new_idx": np.zeros(total, np.int32), "new_x3D": np.zeros((total, 3), np.float32)}
    c = ctx.ptr if ctx is not None else None
    r = lib().cs_object_depth_points(c, int(mode), F, ptr(first), ptr(keys), ptr(_a(has_map_point, np.uint8)), ptr(_a(object_id, np.int32)), ptr(_a(cub_first, np.int32)),
                                     ptr(_a(cuboid_depth, np.float32)), ptr(_a(K4, np.float32)), ptr(_a(bounds, np.float32)), ptr(_a(Twc, np.float32)),
                                     ptr(_a(draw_first, np.int32)), ptr(_a(draws, np.int32)), *[ptr(out[k]) for k in
                                                                                                  ("n_candidates", "raw_depth_pts", "max_initialize_pts", "cand_first", "candidates",
                                                                                                   "shuffled", "new_first", "new_idx", "new_x3D")])
    check(c, r, "cs_object_depth_points")
    nc, nn = int(out["cand_first"][-1]), int(out["new_first"][-1])
    for k in ("n_candidates", "raw_depth_pts", "max_initialize_pts"):
        out[k] = out[k][:F]
    out["candidates"], out["shuffled"], out["new_idx"], out["new_x3D"] = out["candidates"][:nc], out["shuffled"][:nc], out["new_idx"][:nn], out["new_x3D"][:nn]
    return out


def _keys(pts, octave=None):
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    k = np.zeros(len(pts), KEYPOINT_DTYPE)
    k["x"], k["y"], k["class_id"] = pts[:, 0], pts[:, 1], -1
    if octave is not None:
        k["octave"] = octave
    return k


class Tracking:
    """The reference's call sites by name, one key frame (or key-frame pair) per call."""

    @staticmethod
    def MonoObjDepthInitialization(ctx, keysUn, keypoint_associate_objectID, cuboid_depth, K4, Twc):
        """Tracking.cc:876-898: (indices of the key points a MapPoint is created for, in creation order; x3D [n, 3])."""
        keys = keysUn if getattr(keysUn, "dtype", None) == KEYPOINT_DTYPE else _keys(keysUn)
        o = object_depth_points(ctx, FIRST_FRAME, [0, len(keys)], keys, None, keypoint_associate_objectID, [0, len(np.atleast_1d(cuboid_depth))], cuboid_depth, K4, Twc)
        return o["new_idx"], o["new_x3D"]

    @staticmethod
    def CreateNewKeyFrameObjectDepth(ctx, keys, has_map_point, keypoint_associate_objectID, cuboid_depth, K4, bounds, Twc, draws):
        """Tracking.cc:2339-2424 for one key frame; draws = the values rand() returns from here on (at least 80 are enough).  The whole result dict."""
        return object_depth_points(ctx, TRACKING, [0, len(keys)], keys, has_map_point, keypoint_associate_objectID, [0, len(np.atleast_1d(cuboid_depth))], cuboid_depth, K4, Twc,
                                   bounds=bounds, draw_first=[0, len(draws)], draws=draws)

    @staticmethod
    def TriangulateDynamicPoints(ctx, Tcw_last, Tcw_now, K4, cub_pose_last, cub_pose_now, kp1, kp2, obj_last, obj_now, idx_last, world_pos, tracklet_last=None, tracklet_now=None):
        """Tracking.cc:2144-2244 for one key-frame pair: the result dict of triangulate_dynamic_points."""
        n = len(np.asarray(idx_last).reshape(-1))
        return triangulate_dynamic_points(ctx, [0, n], Tcw_last, Tcw_now, K4, [0, len(np.asarray(cub_pose_last).reshape(-1, 7))], cub_pose_last,
                                          [0, len(np.asarray(cub_pose_now).reshape(-1, 7))], cub_pose_now, kp1, kp2, obj_last, obj_now, idx_last, world_pos, tracklet_last,
                                          tracklet_now)


class LocalMapping:
    @staticmethod
    def CreateNewMapPointsObjectDepth(ctx, keys, has_map_point, keypoint_associate_objectID, cuboid_depth, K4, Twc, draws):
        """The tail of LocalMapping::CreateNewMapPoints (LocalMapping.cc:574-652) for one key frame: the whole result dict; new_idx is the order of mlpRecentAddedMapPoints."""
        return object_depth_points(ctx, LOCAL_MAPPING, [0, len(keys)], keys, has_map_point, keypoint_associate_objectID, [0, len(np.atleast_1d(cuboid_depth))], cuboid_depth, K4,
                                   Twc, draw_first=[0, len(draws)], draws=draws)
