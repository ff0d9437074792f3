"""Python host-side mirror of the dynamic-object KLT over the C-ABI: cv::calcOpticalFlowPyrLK as ORBmatcher::SearchByTrackingHarris / SearchByTracking call it
(reference orb_object_slam/src/ORBmatcher.cc:1548 / :1620) and SearchByTrackingHarris itself (:1524-1580), for many frame pairs in one call."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _frames(gray):
    g = np.asarray(gray)
    g = g[None] if g.ndim == 2 else g
    if g.dtype != np.uint8 or g.ndim != 3:
        raise TypeError("frames are uint8 images [F, H, W] or [H, W]")
    if g.strides[2] != 1 or (len(g) > 1 and g.strides[0] != g.strides[1] * g.shape[1]):
        g = np.ascontiguousarray(g)
    return g


def _pairs(pairs, pts):
    """pairs [(prev, next)], pts = one [n, 2] array per pair -> pair_prev, pair_next, first, the points one behind the other."""
    pp = np.ascontiguousarray([a for a, _ in pairs], np.int32)
    pn = np.ascontiguousarray([b for _, b in pairs], np.int32)
    pts = [np.asarray(q, np.float32).reshape(-1, 2) for q in pts]
    if len(pts) != len(pairs):
        raise ValueError("one array of points per pair")
    first = np.zeros(len(pairs) + 1, np.int32)
    first[1:] = np.cumsum([len(q) for q in pts])
    flat = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 2)), np.float32)
    return pp, pn, first, flat


def _outputs(total):
    n = max(total, 1)
    return np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)


def _split(first, *arrays):
    return [tuple(a[first[p]:first[p + 1]].copy() for a in arrays) for p in range(len(first) - 1)]


def _harris_result(first, last, nxt, st, er, kf, kept, kpts, ids, good, outside):
    return [{"kept": kept[kf[p]:kf[p + 1]].copy(), "pts": kpts[kf[p]:kf[p + 1]].copy(), "object_id": ids[kf[p]:kf[p + 1]].copy(), "goodmatches": int(good[p]),
             "n_mask_outside": int(outside[p]), "featuresklt_lastframe": last[first[p]:first[p + 1]].copy(), "featuresklt_thisframe": nxt[first[p]:first[p + 1]].copy(),
             "status": st[first[p]:first[p + 1]].copy(), "err": er[first[p]:first[p + 1]].copy()} for p in range(len(first) - 1)]


def _masks(masks, n_pairs, H, W):
    m = np.ascontiguousarray(masks, np.uint8)
    m = m[None] if m.ndim == 2 else m
    if m.shape != (n_pairs, H, W):
        raise ValueError("one object mask of %s per pair, not %s" % ((H, W), m.shape))
    return m


class KLTTracker:
    """cs_klt wrapper: room for max_frames 8-bit images of at most max_width x max_height and max_points points per call."""

    def __init__(self, max_frames, max_width, max_height, max_points, ctx=None, device=0):
        self.ctx = ctx or _lib.Context(device)
        self._h = C.c_void_p()
        self.W = self.H = self.n_frames = 0
        check(self.ctx.ptr, lib().cs_klt_create(self.ctx.ptr, int(max_frames), int(max_width), int(max_height), int(max_points), C.byref(self._h)), "cs_klt_create")

    def set_frames(self, gray):
        """Pyramids and derivatives of the frames [F, H, W] (or one [H, W]); the rows may be strided."""
        g = _frames(gray)
        check(self.ctx.ptr, lib().cs_klt_set_frames(self.ctx.ptr, self._h, len(g), g.shape[2], g.shape[1], _p(g, C.c_uint8), C.c_long(g.strides[1])), "cs_klt_set_frames")
        self.n_frames, self.H, self.W = g.shape

    @property
    def levels(self):
        return lib().cs_klt_levels(self._h)

    def read_level(self, frame, level):
        """(padded image [h + 42, w + 42] uint8, padded derivatives [h + 42, w + 42, 2] int16) of one resident level."""
        w, h = self.W, self.H
        for _ in range(level):
            w, h = (w + 1) // 2, (h + 1) // 2
        img, der = np.zeros((h + 42, w + 42), np.uint8), np.zeros((h + 42, w + 42, 2), np.int16)
        check(self.ctx.ptr, lib().cs_klt_read_level(self.ctx.ptr, self._h, int(frame), int(level), _p(img, C.c_uint8), _p(der, C.c_int16)), "cs_klt_read_level")
        return img, der

    def track(self, pairs, pts):
        """calcOpticalFlowPyrLK for every pair (prev frame, next frame) of `pairs` over its points: [(nextPts, status, err)] per pair."""
        pp, pn, first, flat = _pairs(pairs, pts)
        nxt, st, er = _outputs(len(flat))
        check(self.ctx.ptr, lib().cs_klt_track(self.ctx.ptr, self._h, len(pp), _p(pp, C.c_int), _p(pn, C.c_int), _p(first, C.c_int), _p(flat if len(flat) else nxt, C.c_float),
                                               _p(nxt, C.c_float), _p(st, C.c_uint8), _p(er, C.c_float)), "cs_klt_track")
        return _split(first, nxt, st, er)

    def search_by_tracking_harris(self, pairs, last_pts, masks):
        """ORBmatcher::SearchByTrackingHarris for every pair: last_pts = pt of LastFrame.mvKeysHarris per pair, masks = CurrentFrame.objmask_img per pair.  Per pair a
        dict of kept (indices into the pair's last_pts, for mvpMapPointsHarris), pts, object_id, goodmatches, n_mask_outside, featuresklt_lastframe /
        featuresklt_thisframe, status, err."""
        pp, pn, first, flat = _pairs(pairs, last_pts)
        m = _masks(masks, len(pp), self.H, self.W)
        n = max(len(flat), 1)
        nxt, st, er = _outputs(len(flat))
        kf, kept, kpts, ids = np.zeros(len(pp) + 1, np.int32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
        good, outside = np.zeros(len(pp), np.int32), np.zeros(len(pp), np.int32)
        check(self.ctx.ptr, lib().cs_match_by_tracking_harris(self.ctx.ptr, self._h, len(pp), _p(pp, C.c_int), _p(pn, C.c_int), _p(first, C.c_int),
                                                              _p(flat if len(flat) else nxt, C.c_float), _p(m, C.c_uint8), _p(nxt, C.c_float), _p(st, C.c_uint8), _p(er, C.c_float),
                                                              _p(kf, C.c_int), _p(kept, C.c_int), _p(kpts, C.c_float), _p(ids, C.c_int), _p(good, C.c_int), _p(outside, C.c_int)),
              "cs_match_by_tracking_harris")
        return _harris_result(first, flat, nxt, st, er, kf, kept, kpts, ids, good, outside)

    def close(self):
        if self._h:
            lib().cs_klt_destroy(self.ctx.ptr, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def calcOpticalFlowPyrLK(frames, pairs, pts, ctx=None):
    """cv::calcOpticalFlowPyrLK(prev, next, pts, Size(21, 21), 3) for the pairs (prev, next) of `frames` [F, H, W]: [(nextPts, status, err)] per pair.  ctx=None: the same
    statement on the host, the comparison side; with a context the device runs it."""
    g = _frames(frames)
    if ctx is not None:
        t = KLTTracker(len(g), g.shape[2], g.shape[1], max(sum(len(np.asarray(q).reshape(-1, 2)) for q in pts), 1), ctx=ctx)
        try:
            t.set_frames(g)
            return t.track(pairs, pts)
        finally:
            t.close()
    pp, pn, first, flat = _pairs(pairs, pts)
    nxt, st, er = _outputs(len(flat))
    check(None, lib().cs_klt_track_host(_p(g, C.c_uint8), len(g), g.shape[2], g.shape[1], C.c_long(g.strides[1]), len(pp), _p(pp, C.c_int), _p(pn, C.c_int), _p(first, C.c_int),
                                        _p(flat if len(flat) else nxt, C.c_float), _p(nxt, C.c_float), _p(st, C.c_uint8), _p(er, C.c_float)), "cs_klt_track_host")
    return _split(first, nxt, st, er)


def SearchByTrackingHarris(frames, pairs, last_pts, masks, ctx=None):
    """ORBmatcher::SearchByTrackingHarris for the pairs (last frame, current frame) of `frames`; see KLTTracker.search_by_tracking_harris.  ctx=None: on the host."""
    g = _frames(frames)
    if ctx is not None:
        t = KLTTracker(len(g), g.shape[2], g.shape[1], max(sum(len(np.asarray(q).reshape(-1, 2)) for q in last_pts), 1), ctx=ctx)
        try:
            t.set_frames(g)
            return t.search_by_tracking_harris(pairs, last_pts, masks)
        finally:
            t.close()
    pp, pn, first, flat = _pairs(pairs, last_pts)
    m = _masks(masks, len(pp), g.shape[1], g.shape[2])
    n = max(len(flat), 1)
    nxt, st, er = _outputs(len(flat))
    kf, kept, kpts, ids = np.zeros(len(pp) + 1, np.int32), np.zeros(n, np.int32), np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
    good, outside = np.zeros(len(pp), np.int32), np.zeros(len(pp), np.int32)
    check(None, lib().cs_match_by_tracking_harris_host(_p(g, C.c_uint8), len(g), g.shape[2], g.shape[1], C.c_long(g.strides[1]), len(pp), _p(pp, C.c_int), _p(pn, C.c_int),
                                                       _p(first, C.c_int), _p(flat if len(flat) else nxt, C.c_float), _p(m, C.c_uint8), _p(nxt, C.c_float), _p(st, C.c_uint8),
                                                       _p(er, C.c_float), _p(kf, C.c_int), _p(kept, C.c_int), _p(kpts, C.c_float), _p(ids, C.c_int), _p(good, C.c_int),
                                                       _p(outside, C.c_int)), "cs_match_by_tracking_harris_host")
    return _harris_result(first, flat, nxt, st, er, kf, kept, kpts, ids, good, outside)


def _tracking_call(fn, head, N, last_keys, eligible, object_id, numobject, th, scale_factors, tail, keys_static, had_map_point, what, ctx_ptr):
    from .orb import KEYPOINT_DTYPE
    lk = np.ascontiguousarray(last_keys, KEYPOINT_DTYPE)
    n_last = len(lk)
    el, ob = np.ascontiguousarray(eligible, np.uint8), np.ascontiguousarray(object_id, np.int32)
    if len(el) != n_last or len(ob) != n_last:
        raise ValueError("one entry per key point of the last frame in eligible and object_id")
    sf = np.ascontiguousarray(scale_factors, np.float32)
    ks = None if keys_static is None else np.ascontiguousarray(keys_static, np.uint8)
    hm = None if had_map_point is None else np.ascontiguousarray(had_map_point, np.uint8)
    for a in (ks, hm):
        if a is not None and len(a) != N:
            raise ValueError("keys_static and had_map_point have one entry per key point of the current frame")
    one = max(n_last, 1)
    train, sel, last, this = np.full(max(N, 1), -1, np.int32), np.zeros(one, np.int32), np.zeros((one, 2), np.float32), np.zeros((one, 2), np.float32)
    n, counters = C.c_int(), np.zeros(4, np.int32)
    pad = lambda a, dt: a if len(a) else np.zeros(1, dt)  # noqa: E731
    check(ctx_ptr, fn(*head, n_last, C.c_void_p(pad(lk, KEYPOINT_DTYPE).ctypes.data), _p(pad(el, np.uint8), C.c_uint8), _p(pad(ob, np.int32), C.c_int), int(numobject), C.c_float(th),
                      _p(sf, C.c_float), len(sf), *tail, None if ks is None else _p(pad(ks, np.uint8), C.c_uint8), None if hm is None else _p(pad(hm, np.uint8), C.c_uint8),
                      _p(train, C.c_int), C.byref(n), _p(sel, C.c_int), _p(last, C.c_float), _p(this, C.c_float), _p(counters, C.c_int)), what)
    k = n.value
    return {"train_match": train[:N], "lastptsinds": sel[:k].copy(), "featuresklt_lastframe": last[:k].copy(), "featuresklt_thisframe": this[:k].copy(),
            "kltmatches": int(counters[0]), "goodmatches": int(counters[1]), "findfeaturematches": int(counters[2]), "uniquematches": int(counters[3])}


def SearchByTracking(last_gray, current_gray, last_keys, eligible, object_id, numobject, th, scale_factors, keysUn, bounds, keys_static=None, had_map_point=None, matcher=None,
                     tracker=None, frames=(0, 1)):
    """ORBmatcher::SearchByTracking (ORBmatcher.cc:1582-1725) for one pair: last_keys = LastFrame.mvKeys (KEYPOINT_DTYPE), eligible[i] = the caller's
    `mvpMapPoints[i] && !KeysStatic[i] && is_dynamic`, object_id = keypoint_associate_objectID; keysUn / bounds / keys_static / had_map_point describe the current
    frame.  Returns a dict: train_match [N] (the last frame's key index whose map point the current key point takes, -1 none), lastptsinds, featuresklt_lastframe /
    featuresklt_thisframe and the four counters.  matcher=None: the same statement on the host.  With an ORBmatcher whose frame is the current frame
    (set_frame / set_frame_from_orb; keysUn and bounds are then not read) the device runs it, through `tracker` (a KLTTracker that holds the two gray frames at
    `frames`) or one made for the call from last_gray / current_gray."""
    from .orb import KEYPOINT_DTYPE
    if matcher is None:
        g = _frames(np.stack([np.asarray(last_gray, np.uint8), np.asarray(current_gray, np.uint8)]))
        ku = np.ascontiguousarray(keysUn, KEYPOINT_DTYPE)
        tail = (C.c_void_p((ku if len(ku) else np.zeros(1, KEYPOINT_DTYPE)).ctypes.data), len(ku), *[C.c_float(float(b)) for b in bounds])
        head = (_p(g[0], C.c_uint8), _p(g[1], C.c_uint8), g.shape[2], g.shape[1], C.c_long(g.strides[1]))
        return _tracking_call(lib().cs_match_by_tracking_host, head, len(ku), last_keys, eligible, object_id, numobject, th, scale_factors, tail, keys_static, had_map_point,
                              "cs_match_by_tracking_host", None)
    own = tracker is None
    if own:
        g = _frames(np.stack([np.asarray(last_gray, np.uint8), np.asarray(current_gray, np.uint8)]))
        tracker = KLTTracker(2, g.shape[2], g.shape[1], max(len(last_keys), 1), ctx=matcher.ctx)
        tracker.set_frames(g)
        frames = (0, 1)
    try:
        head = (matcher.ctx.ptr, matcher._m, tracker._h, int(frames[0]), int(frames[1]))
        return _tracking_call(lib().cs_match_by_tracking, head, matcher.N, last_keys, eligible, object_id, numobject, th, scale_factors, (), keys_static, had_map_point,
                              "cs_match_by_tracking", matcher.ctx.ptr)
    finally:
        if own:
            tracker.close()
