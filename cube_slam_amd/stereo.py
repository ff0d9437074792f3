"""Python host-side mirror of ORB_SLAM2::Frame::ComputeStereoMatches (reference orb_object_slam/src/Frame.cc:611-783) over the C-ABI: the association of
rectified stereo pairs on the device, from what the extractors' last run left there."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Handle, check, lib, ptr
from .orb import KEYPOINT_DTYPE


class StereoMatcher(Handle):
    """cs_stereo wrapper: room for max_pairs pairs of at most max_keypoints_per_frame key points per image."""
    HANDLE, DESTROY = "_s", "cs_stereo_destroy"

    def __init__(self, max_keypoints_per_frame, max_pairs=1, ctx=None, device=0):
        self.ctx = ctx or _lib.Context(device)
        self.cap, self.max_pairs, self.n_pairs = int(max_keypoints_per_frame), int(max_pairs), 0
        self._s = C.c_void_p()
        check(self.ctx.ptr, lib().cs_stereo_create(self.ctx.ptr, self.cap, self.max_pairs, C.byref(self._s)), "cs_stereo_create")

    def match(self, left, right, bf, b, left_first=0, right_first=0, n_pairs=None):
        """Queue the association of n_pairs pairs: frame left_first + p of `left`'s last run against frame right_first + p of `right`'s
        (ORBextractor objects; the same object twice for one run that holds both halves).  Returns at once; results stay on the device."""
        if n_pairs is None:
            n_pairs = left.n_frames - left_first
        check(self.ctx.ptr, lib().cs_stereo_match_from_orb(self.ctx.ptr, self._s, left._e, int(left_first), right._e, int(right_first), int(n_pairs),
                                                           bf, b), "cs_stereo_match_from_orb")
        self.n_pairs = int(n_pairs)

    def match_keys(self, left, right, keysL, descL, keysR, descR, bf, b, left_first=0, right_first=0):
        """The same over host arrays (cs_stereo_match_from_keys): keysL / descL / keysR / descR are lists, one entry per pair, of KEYPOINT_DTYPE arrays and their
        [n, 32] uint8 descriptors.  The extractors supply the pyramids of frames left_first + p / right_first + p of their last run.  A right frame's key points
        must be level-major.  Returns when the arrays have been uploaded; results stay on the device."""
        n_pairs = len(keysL)
        if not (len(descL) == len(keysR) == len(descR) == n_pairs):
            raise ValueError("keysL, descL, keysR and descR are one entry per pair")
        if [len(k) for k in keysL] != [len(d) for d in descL] or [len(k) for k in keysR] != [len(d) for d in descR]:
            raise ValueError("key points and descriptors differ in length")

        def pack(keys, desc):
            first = np.zeros(n_pairs + 1, np.int32)
            first[1:] = np.cumsum([len(k) for k in keys])
            k = np.concatenate([np.asarray(a, KEYPOINT_DTYPE) for a in keys] + [np.zeros(1, KEYPOINT_DTYPE)])  # (one spare record: a pointer that may be handed over)
            d = np.concatenate([np.asarray(a, np.uint8).reshape(-1, 32) for a in desc] + [np.zeros((1, 32), np.uint8)])
            return first, np.ascontiguousarray(k), np.ascontiguousarray(d)
        fL, kL, dL = pack(keysL, descL)
        fR, kR, dR = pack(keysR, descR)
        check(self.ctx.ptr, lib().cs_stereo_match_from_keys(self.ctx.ptr, self._s, left._e, int(left_first), right._e, int(right_first), n_pairs, ptr(fL),
                                                            ptr(kL), ptr(dL), ptr(fR), ptr(kR), ptr(dR), bf, b), "cs_stereo_match_from_keys")
        self.n_pairs = n_pairs

    def read(self):
        """[(mvuRight, mvDepth)] per pair and n_matched[n_pairs]."""
        P = self.n_pairs
        ur = np.zeros((P, self.cap), np.float32)
        dep = np.zeros((P, self.cap), np.float32)
        counts = np.zeros(P, np.int32)
        nm = np.zeros(P, np.int32)
        check(self.ctx.ptr, lib().cs_stereo_read(self.ctx.ptr, self._s, ptr(ur), ptr(dep), self.cap, ptr(counts), ptr(nm)),
              "cs_stereo_read")
        return [(ur[p, :counts[p]].copy(), dep[p, :counts[p]].copy()) for p in range(P)], nm

    def read_packed(self):
        """(mvuRight of every pair one behind the other, mvDepth likewise, first[n_pairs + 1], n_matched) -- two device-to-host copies for the batch."""
        P = self.n_pairs
        first = np.zeros(P + 1, np.int32)
        total = C.c_long()
        check(self.ctx.ptr, lib().cs_stereo_read_packed(self.ctx.ptr, self._s, None, None, 0, ptr(first), C.byref(total), None), "cs_stereo_read_packed")
        ur = np.zeros(max(total.value, 1), np.float32)
        dep = np.zeros(max(total.value, 1), np.float32)
        nm = np.zeros(P, np.int32)
        check(self.ctx.ptr, lib().cs_stereo_read_packed(self.ctx.ptr, self._s, ptr(ur), ptr(dep), len(ur), ptr(first), C.byref(total), ptr(nm)), "cs_stereo_read_packed")
        return ur[:total.value], dep[:total.value], first, nm

    def device_pair(self, pair):
        """(device address of mvuRight, of mvDepth, n) of one pair, for cs_match_fuse / cs_pose_optimization callers that keep it on the device."""
        u, d, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_int()
        check(self.ctx.ptr, lib().cs_stereo_device_pair(self._s, int(pair), C.byref(u), C.byref(d), C.byref(n)), "cs_stereo_device_pair")
        return C.cast(u, C.c_void_p).value, C.cast(d, C.c_void_p).value, n.value


def ComputeStereoMatches(left, right, bf, b, left_first=0, right_first=0, n_pairs=None, matcher=None):
    """Frame::ComputeStereoMatches over two cube_slam_amd.orb.ORBextractor objects after their run(): (mvuRight, mvDepth) as numpy arrays for a single
    pair, a list of such tuples for a batch (n_pairs given, or extractors that hold more than one frame).  `right` may be `left` itself with
    right_first = the first right frame.  bf = mbf, b = mb: the reference sets mb = mbf / fx only after its first call (Frame.cc:141 against :118);
    pass the value meant.  `matcher`: a StereoMatcher to reuse (otherwise one is created for the call)."""
    single = n_pairs is None
    if n_pairs is None:
        n_pairs = left.n_frames - left_first if left is not right else right_first - left_first
    single = single and n_pairs == 1
    m = matcher or StereoMatcher(max(left.cap, right.cap), n_pairs, ctx=left.ctx)
    try:
        m.match(left, right, bf, b, left_first, right_first, n_pairs)
        res, _ = m.read()
    finally:
        if matcher is None:
            m.close()
    return res[0] if single else res
