"""Python host-side mirror of the dynamic-object KLT over the C-ABI: cv::calcOpticalFlowPyrLK as ORBmatcher::SearchByTrackingHarris / SearchByTracking call it
(reference orb_object_slam/src/ORBmatcher.cc:1548 / :1620) and SearchByTrackingHarris itself (:1524-1580), for many frame pairs in one call."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Handle, check, lib, ptr


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


class KLTTracker(Handle):
    """cs_klt wrapper: room for max_frames 8-bit images of at most max_width x max_height and max_points points per call."""
    HANDLE, DESTROY = "_h", "cs_klt_destroy"

    def __init__(self, max_frames, max_width, max_height, max_points, ctx=None, device=0):
        self.ctx = ctx or _lib.Context(device)
        self._h = C.c_void_p()
        self.W = self.H = self.n_frames = 0
        check(self.ctx.ptr, lib().cs_klt_create(self.ctx.ptr, int(max_frames), int(max_width), int(max_height), int(max_points), C.byref(self._h)), "cs_klt_create")

    def set_frames(self, gray):
        """Pyramids and derivatives of the frames [F, H, W] (or one [H, W]); the rows may be strided."""
        g = _frames(gray)
        check(self.ctx.ptr, lib().cs_klt_set_frames(self.ctx.ptr, self._h, len(g), g.shape[2], g.shape[1], ptr(g), g.strides[1]), "cs_klt_set_frames")
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
        check(self.ctx.ptr, lib().cs_klt_read_level(self.ctx.ptr, self._h, int(frame), int(level), ptr(img), ptr(der)), "cs_klt_read_level")
        return img, der

    def track(self, pairs, pts):
        """calcOpticalFlowPyrLK for every pair (prev frame, next frame) of `pairs` over its points: [(nextPts, status, err)] per pair."""
        pp, pn, first, flat = _pairs(pairs, pts)
        nxt, st, er = _outputs(len(flat))
        check(self.ctx.ptr, lib().cs_klt_track(self.ctx.ptr, self._h, len(pp), ptr(pp), ptr(pn), ptr(first), ptr(flat if len(flat) else nxt),
                                               ptr(nxt), ptr(st), ptr(er)), "cs_klt_track")
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
        check(self.ctx.ptr, lib().cs_match_by_tracking_harris(self.ctx.ptr, self._h, len(pp), ptr(pp), ptr(pn), ptr(first),
                                                              ptr(flat if len(flat) else nxt), ptr(m), ptr(nxt), ptr(st), ptr(er),
                                                              ptr(kf), ptr(kept), ptr(kpts), ptr(ids), ptr(good), ptr(outside)),
              "cs_match_by_tracking_harris")
        return _harris_result(first, flat, nxt, st, er, kf, kept, kpts, ids, good, outside)

    def good_features(self, frames, masks, maxCorners, qualityLevel, minDistance):
        """cv::goodFeaturesToTrack on the resident frames `frames` (indices of the last set_frames): masks = one image per frame or None.  Per frame a dict of corners
        [k, 2], quality [k] and n_candidates."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        m = None if masks is None else _masks(masks, len(fr), self.H, self.W)
        out = _gftt_outputs(len(fr), maxCorners)
        r = lib().cs_klt_good_features(self.ctx.ptr, self._h, len(fr), ptr(fr), ptr(m), int(maxCorners), qualityLevel, minDistance, *_gftt_ptrs(out))
        return _gftt_result(self.ctx.ptr, r, "cs_klt_good_features", out)

    def new_harris_features(self, frames, objmasks, exist_pts, exist_obs, K4, Twc, cuboid_depth, good_masks=False):
        """Tracking.cc:2263-2331 on the resident frames `frames`; see NewHarrisFeatures."""
        fr = np.ascontiguousarray(frames, np.int32).reshape(-1)
        a = _harris_args(len(fr), self.H, self.W, objmasks, exist_pts, exist_obs, K4, Twc, cuboid_depth, good_masks)
        r = lib().cs_track_new_harris_features(self.ctx.ptr, self._h, len(fr), ptr(fr), *a["ptrs"])
        return _new_harris_result(self.ctx.ptr, r, "cs_track_new_harris_features", a)


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
    check(None, lib().cs_klt_track_host(ptr(g), len(g), g.shape[2], g.shape[1], g.strides[1], len(pp), ptr(pp), ptr(pn), ptr(first),
                                        ptr(flat if len(flat) else nxt), ptr(nxt), ptr(st), ptr(er)), "cs_klt_track_host")
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
    check(None, lib().cs_match_by_tracking_harris_host(ptr(g), len(g), g.shape[2], g.shape[1], g.strides[1], len(pp), ptr(pp), ptr(pn),
                                                       ptr(first), ptr(flat if len(flat) else nxt), ptr(m), ptr(nxt), ptr(st),
                                                       ptr(er), ptr(kf), ptr(kept), ptr(kpts), ptr(ids), ptr(good), ptr(outside)), "cs_match_by_tracking_harris_host")
    return _harris_result(first, flat, nxt, st, er, kf, kept, kpts, ids, good, outside)


def _gftt_outputs(n, max_corners):
    k = max(int(max_corners), 1)
    return np.zeros((n, k, 2), np.float32), np.zeros((n, k), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)


def _gftt_ptrs(out):
    return [ptr(a) for a in out]


def _gftt_result(ctx_ptr, r, what, out):
    corners, quality, counts, ncand = out
    if r != _lib.CS_OK:
        msg = lib().cs_last_error(ctx_ptr).decode() if ctx_ptr else ""
        e = _lib.CubeSlamError("%s failed: %s %s" % (what, _lib.STATUS.get(r, r), msg))
        e.n_candidates = ncand.copy()  # filled when the call fails with CS_ERR_CAPACITY
        raise e
    return [{"corners": corners[f, :counts[f]].copy(), "quality": quality[f, :counts[f]].copy(), "n_candidates": int(ncand[f])} for f in range(len(counts))]


def _harris_args(n, H, W, objmasks, exist_pts, exist_obs, K4, Twc, cuboid_depth, good_masks):
    m = _masks(objmasks, n, H, W)
    pts = [np.asarray(q, np.float32).reshape(-1, 2) for q in exist_pts]
    obs = [np.asarray(o, np.int32).reshape(-1) for o in exist_obs]
    dep = [np.asarray(d, np.float32).reshape(-1) for d in cuboid_depth]
    if len(pts) != n or len(obs) != n or len(dep) != n or any(len(q) != len(o) for q, o in zip(pts, obs)):
        raise ValueError("one array of points, of observation counts and of cuboid depths per frame")
    ef, cf = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    ef[1:], cf[1:] = np.cumsum([len(q) for q in pts]), np.cumsum([len(d) for d in dep])
    cat = lambda a, shape, dt: np.ascontiguousarray(np.concatenate(a) if a else np.zeros(shape, dt), dt)  # noqa: E731
    fp, fo, fd = cat(pts, (0, 2), np.float32), cat(obs, 0, np.int32), cat(dep, 0, np.float32)
    pad = lambda a: a if a.size else np.zeros(2, a.dtype)  # noqa: E731
    fp, fo, fd = pad(fp), pad(fo), pad(fd)
    k4 = np.ascontiguousarray(K4, np.float32).reshape(4)
    T = np.ascontiguousarray(np.asarray(Twc, np.float32).reshape(n, -1)[:, :12])
    cap = 200 * n
    o = {"new_first": np.zeros(n + 1, np.int32), "pts": np.zeros((cap, 2), np.float32), "object_id": np.zeros(cap, np.int32), "x3D": np.zeros((cap, 3), np.float32),
         "x3D_valid": np.zeros(cap, np.uint8), "n_mask_outside": np.zeros(n, np.int32), "good": np.zeros((n, H, W), np.uint8) if good_masks else None,
         "n_candidates": np.zeros(n, np.int32)}
    o["keep"] = (m, fp, fo, fd, k4, T, ef, cf)
    o["ptrs"] = (ptr(m), ptr(ef), ptr(fp), ptr(fo), ptr(k4), ptr(T), ptr(cf), ptr(fd),
                 ptr(o["new_first"]), ptr(o["pts"]), ptr(o["object_id"]), ptr(o["x3D"]), ptr(o["x3D_valid"]),
                 ptr(o["n_mask_outside"]), ptr(o["good"]), ptr(o["n_candidates"]))
    return o


def _new_harris_result(ctx_ptr, r, what, a):
    if r != _lib.CS_OK:
        msg = lib().cs_last_error(ctx_ptr).decode() if ctx_ptr else ""
        e = _lib.CubeSlamError("%s failed: %s %s" % (what, _lib.STATUS.get(r, r), msg))
        e.n_candidates = a["n_candidates"].copy()
        raise e
    nf = a["new_first"]
    out = []
    for f in range(len(nf) - 1):
        d = {k: a[k][nf[f]:nf[f + 1]].copy() for k in ("pts", "object_id", "x3D", "x3D_valid")}
        d["n_mask_outside"], d["n_candidates"] = int(a["n_mask_outside"][f]), int(a["n_candidates"][f])
        if a["good"] is not None:
            d["good"] = a["good"][f].copy()
        out.append(d)
    return out


def goodFeaturesToTrack(frames, masks, maxCorners, qualityLevel, minDistance, ctx=None):
    """cv::goodFeaturesToTrack(frame, corners, maxCorners, qualityLevel, minDistance, mask) with blockSize 3 and the minimum eigenvalue, for every image of `frames`
    [F, H, W] (or one [H, W]); masks = one image per frame or None.  Per frame a dict of corners [k, 2], quality [k] (the thresholded eigenvalue) and n_candidates.
    ctx=None: the same statement on the host, the comparison side; with a context the device runs it."""
    g = _frames(frames)
    m = None if masks is None else _masks(masks, len(g), g.shape[1], g.shape[2])
    out = _gftt_outputs(len(g), maxCorners)
    head = (ptr(g), len(g), g.shape[2], g.shape[1], g.strides[1], ptr(m), int(maxCorners), qualityLevel, minDistance)
    if ctx is not None:
        return _gftt_result(ctx.ptr, lib().cs_good_features_images(ctx.ptr, *head, *_gftt_ptrs(out)), "cs_good_features_images", out)
    return _gftt_result(None, lib().cs_klt_good_features_host(*head, *_gftt_ptrs(out)), "cs_klt_good_features_host", out)


def NewHarrisFeatures(frames, objmasks, exist_pts, exist_obs, K4, Twc, cuboid_depth, ctx=None, good_masks=False):
    """The new-feature loop of Tracking::CreateNewKeyFrame (Tracking.cc:2263-2331) for every image of `frames`: objmasks = objmask_img per frame, exist_pts / exist_obs =
    per frame the pt and Observations() of the existing dynamic points, K4 = (fx, fy, cx, cy), Twc = the key frames' poses ([F, 3, 4] or [F, 4, 4]), cuboid_depth = per
    frame the camera z of its local cuboids.  Per frame a dict of pts, object_id, x3D, x3D_valid, n_mask_outside, n_candidates (and good, the mask that was built, with
    good_masks=True).  ctx=None: on the host."""
    g = _frames(frames)
    if ctx is not None:
        t = KLTTracker(len(g), g.shape[2], g.shape[1], 1, ctx=ctx)
        try:
            t.set_frames(g)
            return t.new_harris_features(np.arange(len(g)), objmasks, exist_pts, exist_obs, K4, Twc, cuboid_depth, good_masks)
        finally:
            t.close()
    a = _harris_args(len(g), g.shape[1], g.shape[2], objmasks, exist_pts, exist_obs, K4, Twc, cuboid_depth, good_masks)
    r = lib().cs_track_new_harris_features_host(ptr(g), len(g), g.shape[2], g.shape[1], g.strides[1], *a["ptrs"])
    return _new_harris_result(None, r, "cs_track_new_harris_features_host", a)


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
    check(ctx_ptr, fn(*head, n_last, ptr(pad(lk, KEYPOINT_DTYPE)), ptr(pad(el, np.uint8)), ptr(pad(ob, np.int32)), int(numobject), th,
                      ptr(sf), len(sf), *tail, None if ks is None else ptr(pad(ks, np.uint8)), None if hm is None else ptr(pad(hm, np.uint8)),
                      ptr(train), C.byref(n), ptr(sel), ptr(last), ptr(this), ptr(counters)), what)
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
        tail = (ptr(ku if len(ku) else np.zeros(1, KEYPOINT_DTYPE)), len(ku), *[float(b) for b in bounds])
        head = (ptr(g[0]), ptr(g[1]), g.shape[2], g.shape[1], g.strides[1])
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
