"""GPU parity of cv::goodFeaturesToTrack (cs_klt_good_features on resident frames, cs_good_features_images on passed images) and of the new-Harris-feature loop of
Tracking::CreateNewKeyFrame (cs_track_new_harris_features, Tracking.cc:2263-2331) through the C-ABI against tests/gftt_restatement.py, byte for byte on corners and
their order, quality, counts, n_candidates, the masks that were built, object ids, x3D, x3D_valid and n_mask_outside.  No tolerance anywhere: every sum has its order
and its roundings.  tests/test_gftt_patterns.py asserts on the restatement that the inputs take every branch."""
import ctypes as C

import numpy as np
import pytest

from cube_slam_amd import _lib
from cube_slam_amd.klt import KLTTracker, NewHarrisFeatures, goodFeaturesToTrack
from tests import gftt_patterns as gp
from tests import gftt_restatement as gr

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD_ARG, CAPACITY = -2, -4


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _device(ctx, c):
    """The case on the device: on the image itself and, where a KLT handle takes the size, on a resident frame (between two other frames, so its slot is not 0)."""
    mask = None if c["mask"] is None else c["mask"][None]
    got = [goodFeaturesToTrack(c["img"], mask, c["max_corners"], c["quality"], c["min_distance"], ctx=ctx)[0]]
    h, w = c["img"].shape
    if w > 21 and h > 21:
        t = KLTTracker(3, w, h, 1, ctx=ctx)
        try:
            t.set_frames(np.stack([np.zeros_like(c["img"]), c["img"], c["img"][::-1]]))
            got.append(t.good_features([1], mask, c["max_corners"], c["quality"], c["min_distance"])[0])
        finally:
            t.close()
    return got


@pytest.mark.parametrize("w,h", gp.SIZES)
def test_good_features_at_every_size(ctx, w, h):
    c = gp.size_case(w, h)
    for g in _device(ctx, c):
        assert gp.same_features(g, c["want"])
    if c["mask"] is not None:  # the NULL mask
        assert gp.same_features(goodFeaturesToTrack(c["img"], None, 200, 0.05, 3.0, ctx=ctx)[0], gr.good_features(c["img"], None, 200, 0.05, 3.0))


@pytest.mark.parametrize("name", sorted(gp.designed_cases()))
def test_good_features_on_designed_cases(ctx, name):
    c = gp.designed_cases()[name]
    for g in _device(ctx, c):
        assert gp.same_features(g, c["want"]), (len(g["corners"]), len(c["want"]["corners"]), g["n_candidates"], c["want"]["n_candidates"])
    if name == "border_corner":
        assert not gp.same_features(_device(ctx, c)[0], c["image_variant"])


def test_batch_in_one_call_and_one_frame_per_call(ctx):
    b = gp.batch_case()
    n, h, w = b["frames"].shape
    t = KLTTracker(n, w, h, 1, ctx=ctx)
    try:
        t.set_frames(b["frames"])
        got = t.good_features(np.arange(n), None, 200, 0.1, 5.0)
        assert [len(g["corners"]) for g in got] == [0, 1, 199, 200, 200]
        assert all(gp.same_features(g, c["want"]) for g, c in zip(got, b["cases"]))
        for f in (4, 2, 0, 3, 1):
            assert gp.same_features(t.good_features([f], None, 200, 0.1, 5.0)[0], b["cases"][f]["want"]), f
        twice = t.good_features([3, 3, 1], None, 200, 0.1, 5.0)  # a frame may be named twice
        assert gp.same_features(twice[0], b["cases"][3]["want"]) and gp.same_features(twice[1], b["cases"][3]["want"]) and gp.same_features(twice[2], b["cases"][1]["want"])
        few = t.good_features([4], None, 7, 0.1, 5.0)[0]         # the stop inside the first batch
        assert few["corners"].tobytes() == b["cases"][4]["want"]["corners"][:7].tobytes()
    finally:
        t.close()
    assert all(gp.same_features(g, c["want"]) for g, c in zip(goodFeaturesToTrack(b["frames"], None, 200, 0.1, 5.0, ctx=ctx), b["cases"]))


def test_capacity_seam_reuse_and_errors(ctx):
    """CS_GFTT_MAX_CANDIDATES candidates are sorted and walked; one more is CS_ERR_CAPACITY with the count filled.  The handle then takes a smaller size and every
    argument error, and still answers."""
    full, over, small = gp.capacity_case(0), gp.capacity_case(1), gp.size_case(64, 48)
    h, w = full["img"].shape
    t = KLTTracker(2, w, h, 1, ctx=ctx)
    L = _lib.lib()
    try:
        t.set_frames(np.stack([full["img"], over["img"]]))
        assert gp.same_features(t.good_features([0], None, 200, 0.1, 10.0)[0], full["want"])
        with pytest.raises(_lib.CubeSlamError, match="CS_ERR_CAPACITY") as e:
            t.good_features([0, 1], None, 200, 0.1, 10.0)
        assert list(e.value.n_candidates) == [gr.MAX_CANDIDATES, gr.MAX_CANDIDATES + 1]
        assert gp.same_features(t.good_features([0], None, 200, 0.1, 10.0)[0], full["want"])      # ... and the handle still answers
        t.set_frames(small["img"])                                                                # a smaller size within the capacity
        assert gp.same_features(t.good_features([0], small["mask"][None], 200, small["quality"], small["min_distance"])[0], small["want"])
        corners, quality, counts, ncand = np.zeros((200, 2), f32), np.zeros(200, f32), np.zeros(1, np.int32), np.zeros(1, np.int32)
        fr = np.zeros(1, np.int32)

        def call(frames=fr, n=1, mc=200, q=0.1, md=10.0, c=corners, cnt=counts):
            return L.cs_klt_good_features(ctx.ptr, t._h, n, None if frames is None else _p(frames, C.c_int), None, mc, C.c_double(q), C.c_double(md),
                                          None if c is None else _p(c, C.c_float), _p(quality, C.c_float), None if cnt is None else _p(cnt, C.c_int), _p(ncand, C.c_int))
        assert call() == 0
        assert call(frames=np.ones(1, np.int32)) == BAD_ARG and call(frames=-np.ones(1, np.int32)) == BAD_ARG     # frame 1 is no longer set
        assert call(mc=0) == BAD_ARG and call(md=0.99) == BAD_ARG and call(q=0.0) == BAD_ARG and call(q=1.01) == BAD_ARG and call(q=float("nan")) == BAD_ARG
        assert call(frames=None) == BAD_ARG and call(n=0) == BAD_ARG and call(c=None) == BAD_ARG and call(cnt=None) == BAD_ARG
        assert gp.same_features(t.good_features([0], small["mask"][None], 200, small["quality"], small["min_distance"])[0], small["want"])
        fresh = KLTTracker(1, 64, 48, 1, ctx=ctx)
        try:
            with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
                fresh.good_features([0], None, 200, 0.1, 10.0)                                     # no frames are set
        finally:
            fresh.close()
    finally:
        t.close()
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_CAPACITY"):
        goodFeaturesToTrack(over["img"], None, 200, 0.1, 10.0, ctx=ctx)


def _harris(t, cases, frames):
    return t.new_harris_features(frames, [c["objmask"] for c in cases], [c["pts"] for c in cases], [c["obs"] for c in cases], gp.K4, np.stack([gp.TWC] * len(cases)),
                                 [c["depth"] for c in cases], good_masks=True)


def test_new_harris_features(ctx):
    """Every mask-building and new-point case, all in one call (each frame resident once, named in another order than it was set) and one per call."""
    names = sorted(gp.harris_cases())
    cases = [gp.harris_cases()[k] for k in names]
    t = KLTTracker(len(cases), gp.MW, gp.MH, 1, ctx=ctx)
    try:
        t.set_frames(np.stack([c["img"] for c in cases]))
        order = list(range(len(cases)))[::-1]
        got = _harris(t, [cases[i] for i in order], order)
        for i, g in zip(order, got):
            assert gp.same_harris(g, cases[i]["want"]), names[i]
        for i in order:
            assert gp.same_harris(_harris(t, [cases[i]], [i])[0], cases[i]["want"]), names[i]
        # an object without a cuboid: CS_ERR_BAD_ARG, also when another frame of the call is fine; existing points that are not finite; then the handle answers again
        missing, base = gp.depth_case("missing"), gp.mask_edge_case()
        t.set_frames(np.stack([missing["img"], base["img"]]))
        with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
            _harris(t, [base, missing], [1, 0])
        bad = dict(base, pts=base["pts"].copy())
        bad["pts"][0, 1] = np.nan
        with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
            _harris(t, [bad], [1])
        with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG"):
            _harris(t, [base], [2])                                                                # no such frame
        assert gp.same_harris(_harris(t, [base], [1])[0], base["want"])
    finally:
        t.close()
    c = gp.mask_edge_case()
    got = NewHarrisFeatures(c["img"], [c["objmask"]], [c["pts"]], [c["obs"]], c["K4"], c["Twc"][None], [c["depth"]], ctx=ctx, good_masks=True)[0]
    assert gp.same_harris(got, c["want"])


def test_new_harris_features_at_the_capacity_seam(ctx):
    """The lattice of 8 192 equal dots under an object mask: the candidates fill the capacity, 200 are taken; with one dot more the call is CS_ERR_CAPACITY."""
    full, over = gp.capacity_case(0), gp.capacity_case(1)
    h, w = full["img"].shape
    obj = np.ones((h, w), np.uint8)
    want = gr.new_harris_features(full["img"], obj, np.zeros((0, 2), f32), [], gp.K4, gp.TWC, [2.0])
    assert want["n_candidates"] == gr.MAX_CANDIDATES and len(want["pts"]) == 200
    got = NewHarrisFeatures(full["img"], [obj], [[]], [[]], gp.K4, gp.TWC[None], [[2.0]], ctx=ctx, good_masks=True)[0]
    assert gp.same_harris(got, want)
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_CAPACITY") as e:
        NewHarrisFeatures(over["img"], [obj], [[]], [[]], gp.K4, gp.TWC[None], [[2.0]], ctx=ctx)
    assert e.value.n_candidates[0] == gr.MAX_CANDIDATES + 1


def test_tracking_create_new_harris_features(ctx):
    from cube_slam_amd.tracking import Tracking
    c = gp.mask_order_case(1)
    pts, ids, obj, x3D, r = object.__new__(Tracking).CreateNewHarrisFeatures(c["img"], c["objmask"], c["pts"], [3, 4], c["obs"], [0, 0], c["K4"], c["Twc"], c["depth"], next_point_id=50,
                                                                             ctx=ctx)
    k = len(c["want"]["pts"])
    assert pts[2:].tobytes() == c["want"]["pts"].tobytes() and list(ids) == [3, 4] + list(range(50, 50 + k)) and x3D.tobytes() == c["want"]["x3D"].tobytes()
    assert list(obj[2:]) == list(c["want"]["object_id"])
