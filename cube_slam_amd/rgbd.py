"""Python host-side mirror of ORB_SLAM2::Frame::ComputeStereoFromRGBD (reference orb_object_slam/src/Frame.cc:785-806) and of the rule by which Tracking creates map
points from measured depth (src/Tracking.cc:783-850, :1207-1274, :2067-2130 over Frame::UnprojectStereo, Frame.cc:808-822) over the C-ABI."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Handle, check, lib, ptr
from .orb import KEYPOINT_DTYPE

CS_DEPTH_U16, CS_DEPTH_F32 = 0, 1
CS_RGBD_MAX_KEYPOINTS = 8192
CS_CLOSE_POINTS_NEAREST, CS_CLOSE_POINTS_ALL = 0, 1


def _depth_type(a):
    if a.dtype == np.uint16:
        return CS_DEPTH_U16
    if a.dtype == np.float32:
        return CS_DEPTH_F32
    raise TypeError("a depth image is uint16 (the sensor's units) or float32, not %s" % a.dtype)


def _keys(a):
    a = np.ascontiguousarray(a, KEYPOINT_DTYPE)
    return a if len(a) else np.zeros(1, KEYPOINT_DTYPE)  # (a pointer that may be handed over; no record of it is read)


def _close_points_raw(fn, head, first, need_new, Tcw, K4, th_depth, mode, what, ctx_ptr):
    """The common tail of cs_close_points / cs_rgbd_close_points as the C-ABI returns it: (first, n_valid, order, n_walked, new_first, new_idx, new_x3D)."""
    first = np.ascontiguousarray(first, np.int32)
    F, total = len(first) - 1, int(first[-1])
    Tcw = np.ascontiguousarray(np.asarray(Tcw, np.float32).reshape(F, -1)[:, :12])
    K4 = np.ascontiguousarray(K4, np.float32)
    need = None if need_new is None else np.ascontiguousarray(need_new, np.uint8)
    if need is not None and len(need) != total:
        raise ValueError("need_new has %d entries for %d key points" % (len(need), total))
    n_valid, n_walked, new_first = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F + 1, np.int32)
    order, new_idx, new_x3D = np.empty(max(total, 1), np.int32), np.empty(max(total, 1), np.int32), np.empty((max(total, 1), 3), np.float32)
    check(ctx_ptr, fn(*head, None if need is None else ptr(need if len(need) else np.zeros(1, np.uint8)), ptr(Tcw),
                      ptr(K4), th_depth, int(mode), ptr(n_valid), ptr(order), ptr(n_walked), ptr(new_first), ptr(new_idx), ptr(new_x3D)), what)
    return first, n_valid, order, n_walked, new_first, new_idx, new_x3D


def _close_points_call(*args):
    """... and per frame a dict of n_valid, order, n_walked, new_idx, new_x3D."""
    first, n_valid, order, n_walked, new_first, new_idx, new_x3D = _close_points_raw(*args)
    return [{"n_valid": int(n_valid[f]), "order": order[first[f]:first[f] + n_valid[f]].copy(), "n_walked": int(n_walked[f]),
             "new_idx": new_idx[new_first[f]:new_first[f + 1]].copy(), "new_x3D": new_x3D[new_first[f]:new_first[f + 1]].copy()} for f in range(len(first) - 1)]


class RGBDAssociator(Handle):
    """cs_rgbd wrapper: room for max_frames depth images of width x height and at most max_keypoints_per_frame key points per frame."""
    HANDLE, DESTROY = "_h", "cs_rgbd_destroy"

    def __init__(self, width, height, max_keypoints_per_frame, max_frames=1, ctx=None, device=0):
        self.ctx = ctx or _lib.Context(device)
        self.W, self.H, self.cap, self.max_frames, self.n_frames = int(width), int(height), int(max_keypoints_per_frame), int(max_frames), 0
        self._h = C.c_void_p()
        check(self.ctx.ptr, lib().cs_rgbd_create(self.ctx.ptr, self.W, self.H, self.cap, self.max_frames, C.byref(self._h)), "cs_rgbd_create")

    def upload_depth(self, depth):
        """Depth images [F, H, W] or [H, W], uint16 or float32, stored raw; the rows may be strided (a view of a wider buffer)."""
        d = np.asarray(depth)
        d = d[None] if d.ndim == 2 else d
        if d.shape[1:] != (self.H, self.W):
            raise ValueError("depth images of %s for a handle of %s" % (d.shape[1:], (self.H, self.W)))
        if d.strides[2] != d.itemsize or (len(d) > 1 and d.strides[0] != d.strides[1] * self.H):
            d = np.ascontiguousarray(d)
        self._depth = d  # (the copy is asynchronous)
        check(self.ctx.ptr, lib().cs_rgbd_upload_depth(self.ctx.ptr, self._h, ptr(d), _depth_type(d), len(d), d.strides[1]), "cs_rgbd_upload_depth")

    def set_depth_device(self, address, dtype, n_frames):
        """A dense depth batch already in device memory (its address as an int, e.g. torch.Tensor.data_ptr())."""
        check(self.ctx.ptr, lib().cs_rgbd_set_depth_device(self.ctx.ptr, self._h, int(address), _depth_type(np.empty(0, dtype)), int(n_frames)), "cs_rgbd_set_depth_device")

    def from_orb(self, orb, K4, dist5, bf, depth_map_factor=1.0, first_frame=0, n_frames=None):
        """Queue ComputeStereoFromRGBD for frames first_frame .. of `orb`'s last run (an ORBextractor) against the uploaded depth images.  Returns at once."""
        if n_frames is None:
            n_frames = orb.n_frames - first_frame
        K4 = np.ascontiguousarray(K4, np.float32)
        d5 = None if dist5 is None else np.ascontiguousarray(dist5, np.float32)
        check(self.ctx.ptr, lib().cs_rgbd_from_orb(self.ctx.ptr, self._h, orb._e, int(first_frame), int(n_frames), ptr(K4), ptr(d5), bf, depth_map_factor),
              "cs_rgbd_from_orb")
        self.n_frames = int(n_frames)

    def from_keys(self, keys, keysUn, bf, depth_map_factor=1.0):
        """The same over host arrays: keys / keysUn are lists (one entry per frame) of KEYPOINT_DTYPE arrays, mvKeys and mvKeysUn."""
        first = np.zeros(len(keys) + 1, np.int32)
        first[1:] = np.cumsum([len(k) for k in keys])
        k = _keys(np.concatenate([np.asarray(a, KEYPOINT_DTYPE) for a in keys]) if len(keys) else [])
        ku = _keys(np.concatenate([np.asarray(a, KEYPOINT_DTYPE) for a in keysUn]) if len(keysUn) else [])
        if [len(a) for a in keys] != [len(a) for a in keysUn]:
            raise ValueError("mvKeys and mvKeysUn differ in length")
        check(self.ctx.ptr, lib().cs_rgbd_from_keys(self.ctx.ptr, self._h, len(keys), ptr(first), ptr(k), ptr(ku), bf, depth_map_factor), "cs_rgbd_from_keys")
        self.n_frames = len(keys)

    def read(self):
        """[(mvuRight, mvDepth)] per frame, n_with_depth[n_frames], n_outside[n_frames]."""
        F = self.n_frames
        ur, dep = np.zeros((F, self.cap), np.float32), np.zeros((F, self.cap), np.float32)
        counts, nd, no = np.zeros(F, np.int32), np.zeros(F, np.int32), np.zeros(F, np.int32)
        check(self.ctx.ptr, lib().cs_rgbd_read(self.ctx.ptr, self._h, ptr(ur), ptr(dep), self.cap, ptr(counts), ptr(nd), ptr(no)),
              "cs_rgbd_read")
        return [(ur[f, :counts[f]].copy(), dep[f, :counts[f]].copy()) for f in range(F)], nd, no

    def read_packed(self):
        """(mvuRight of every frame one behind the other, mvDepth likewise, first[n_frames + 1], n_with_depth, n_outside)."""
        F = self.n_frames
        first = np.zeros(F + 1, np.int32)
        total = C.c_long()
        check(self.ctx.ptr, lib().cs_rgbd_read_packed(self.ctx.ptr, self._h, None, None, 0, ptr(first), C.byref(total), None, None), "cs_rgbd_read_packed")
        ur, dep = np.zeros(max(total.value, 1), np.float32), np.zeros(max(total.value, 1), np.float32)
        nd, no = np.zeros(F, np.int32), np.zeros(F, np.int32)
        check(self.ctx.ptr, lib().cs_rgbd_read_packed(self.ctx.ptr, self._h, ptr(ur), ptr(dep), len(ur), ptr(first), C.byref(total),
                                                      ptr(nd), ptr(no)), "cs_rgbd_read_packed")
        return ur[:total.value], dep[:total.value], first, nd, no

    def read_keys_un(self):
        """mvKeysUn of every frame one behind the other (read_packed's order)."""
        first = np.zeros(self.n_frames + 1, np.int32)
        total = C.c_long()
        check(self.ctx.ptr, lib().cs_rgbd_read_packed(self.ctx.ptr, self._h, None, None, 0, ptr(first), C.byref(total), None, None), "cs_rgbd_read_packed")
        ku = np.zeros(max(total.value, 1), KEYPOINT_DTYPE)
        check(self.ctx.ptr, lib().cs_rgbd_read_keys_un(self.ctx.ptr, self._h, ptr(ku), len(ku)), "cs_rgbd_read_keys_un")
        return ku[:total.value]

    def device_frame(self, frame):
        """(device address of mvuRight, of mvDepth, of mvKeysUn, n) of one frame, for cs_match_fuse / cs_pose_optimization callers that keep it on the device."""
        u, d, k, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_void_p(), C.c_int()
        check(self.ctx.ptr, lib().cs_rgbd_device_frame(self._h, int(frame), C.byref(u), C.byref(d), C.byref(k), C.byref(n)), "cs_rgbd_device_frame")
        return C.cast(u, C.c_void_p).value, C.cast(d, C.c_void_p).value, k.value, n.value

    def close_points(self, need_new, Tcw, K4, th_depth, mode=CS_CLOSE_POINTS_NEAREST, raw=False):
        """The close-point rule on what the last from_orb / from_keys left on the device: need_new over all frames' key points one behind the other (None with
        CS_CLOSE_POINTS_ALL), Tcw [n_frames, 3, 4].  Per frame a dict of n_valid, order, n_walked, new_idx (in creation order) and new_x3D; raw=True: the arrays of the
        C-ABI instead (first, n_valid, order, n_walked, new_first, new_idx, new_x3D)."""
        first = np.zeros(self.n_frames + 1, np.int32)
        total = C.c_long()
        check(self.ctx.ptr, lib().cs_rgbd_read_packed(self.ctx.ptr, self._h, None, None, 0, ptr(first), C.byref(total), None, None), "cs_rgbd_read_packed")
        return (_close_points_raw if raw else _close_points_call)(lib().cs_rgbd_close_points, (self.ctx.ptr, self._h), first, need_new, Tcw, K4, th_depth, mode,
                                                                  "cs_rgbd_close_points", self.ctx.ptr)


def ComputeStereoFromRGBD(imDepth, keys, keysUn, bf, depth_map_factor=1.0, ctx=None, counts=False):
    """Frame::ComputeStereoFromRGBD for one frame: imDepth [H, W] uint16 or float32 as the sensor gave it (the convertTo of Tracking.cc:388 is depth_map_factor), keys /
    keysUn = mvKeys / mvKeysUn (KEYPOINT_DTYPE).  Returns (mvuRight, mvDepth), with counts=True also (n_with_depth, n_outside).  ctx=None: the same statement on the
    host, the comparison side; with a context the device runs it."""
    d = np.asarray(imDepth)
    H, W = d.shape
    n = len(keys)
    if ctx is not None:
        a = RGBDAssociator(W, H, max(n, 1), 1, ctx=ctx)
        try:
            a.upload_depth(d)
            a.from_keys([keys], [keysUn], bf, depth_map_factor)
            res, nd, no = a.read()
        finally:
            a.close()
        return res[0] + ((int(nd[0]), int(no[0])),) if counts else res[0]
    if d.strides[1] != d.itemsize:
        d = np.ascontiguousarray(d)
    k, ku = _keys(keys), _keys(keysUn)
    ur, dep = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    nd, no = C.c_int(), C.c_int()
    check(None, lib().cs_rgbd_host_from_keys(ptr(d), _depth_type(d), W, H, d.strides[0], n, ptr(k), ptr(ku),
                                             bf, depth_map_factor, ptr(ur), ptr(dep), C.byref(nd), C.byref(no)), "cs_rgbd_host_from_keys")
    return (ur[:n], dep[:n], (nd.value, no.value)) if counts else (ur[:n], dep[:n])


def ClosePoints(depth, keysUn, need_new, Tcw, K4, th_depth, mode=CS_CLOSE_POINTS_NEAREST, first=None, ctx=None):
    """The close-point rule of Tracking::UpdateLastFrame / CreateNewKeyFrame (mode CS_CLOSE_POINTS_NEAREST) and StereoInitialization (CS_CLOSE_POINTS_ALL) over
    mvDepth from any source.  One frame (first=None: depth, keysUn, need_new of that frame, Tcw [3, 4]; returns a dict) or several one behind the other (first =
    n_frames + 1 offsets, Tcw [n_frames, 3, 4]; returns a list of dicts): n_valid, order, n_walked, new_idx in creation order, new_x3D.  ctx=None: on the host."""
    single = first is None
    depth = np.ascontiguousarray(depth, np.float32)
    if single:
        first = [0, len(depth)]
    ku = _keys(keysUn)
    cp = None if ctx is None else ctx.ptr
    res = _close_points_call(lib().cs_close_points, (cp, len(first) - 1, ptr(np.ascontiguousarray(first, np.int32)), ptr(depth if len(depth) else np.zeros(1, np.float32)),
                                                     ptr(ku)), first, need_new, Tcw, K4, th_depth, mode, "cs_close_points", cp)
    return res[0] if single else res
