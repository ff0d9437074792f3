"""GPU parity of the RGB-D association (cs_rgbd_*, Frame::ComputeStereoFromRGBD, Frame.cc:785-806) and of the close-point rule (cs_close_points /
cs_rgbd_close_points; Tracking.cc:783-850, :1207-1274, :2067-2130) through the C-ABI against tests/rgbd_restatement.py, byte for byte.  No tolerance anywhere: every
operation is a single float operation in a fixed order or a double accumulation with one rounding.  Shares are asserted so that an all -1 / nothing-created answer on
both sides cannot pass: full frames of the gather generator have 70.3 - 87.3 % of their key points with depth (tests/test_rgbd_restatement.py prints them; the band
here is that range widened by 0.1), and every close-point call holds frames that create some but not all of their points."""
import ctypes as C

import numpy as np
import pytest

from cube_slam_amd import _lib
from cube_slam_amd.orb import KEYPOINT_DTYPE, ORBextractor
from cube_slam_amd.rgbd import CS_CLOSE_POINTS_ALL, CS_CLOSE_POINTS_NEAREST, CS_RGBD_MAX_KEYPOINTS, ClosePoints, ComputeStereoFromRGBD, RGBDAssociator
from cube_slam_amd.tracking import Tracking
from tests import rgbd_restatement as rr
from tests import stereo_restatement as sr

pytestmark = pytest.mark.gpu
f32 = np.float32
BAD_ARG, CAPACITY = -2, -4
SHARE_LO, SHARE_HI = 0.60, 0.97
CP_W, CP_H, CP_CAP = 128, 64, 2048  # the close-point frames: one pixel per key point, a handle capacity above one pass of the kernel's 1 024 threads


class _Dev:
    def __init__(self, ptr, n, typestr="<f4"):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def _same_close(got, want, what):
    assert got["n_valid"] == want["n_valid"] and got["n_walked"] == want["n_walked"], (what, got["n_valid"], want["n_valid"], got["n_walked"], want["n_walked"])
    for key in ("order", "new_idx", "new_x3D"):
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (what, key)


@pytest.mark.parametrize("dt,factor", [(np.uint16, rr.FACTOR), (np.float32, 1.0)])
def test_gather_from_keys_equals_restatement(ctx, dt, factor):
    """Frames of 64, 0, 257, 1, 63, 65 key points and the frame of edge cases in one call over a 64 x 48 image with TUM1's distortion."""
    W, H = 64, 48
    K = rr.small_K4(W, H)
    sizes = rr.FRAME_SIZES
    images = [rr.depth_image(3, W, H, dt)] * len(sizes) + [rr.edge_image(W, H, dt)]
    keys = [rr.keypoints(n + 5, n, W, H) for n in sizes] + [rr.edge_keypoints(W, H)]
    keysUn = [rr.undistort_keypoints(k, K, rr.DIST5) for k in keys]
    a = RGBDAssociator(W, H, max(sizes), len(keys), ctx=ctx)
    a.upload_depth(np.stack(images))
    a.from_keys(keys, keysUn, rr.BF, factor)
    got, n_with, n_out = a.read()
    pu, pd, first, pn_with, pn_out = a.read_packed()
    assert np.array_equal(first, np.concatenate([[0], np.cumsum([len(k) for k in keys])])) and np.array_equal(pn_with, n_with) and np.array_equal(pn_out, n_out)
    assert a.read_keys_un().tobytes() == np.concatenate(keysUn).tobytes()
    for f, (im, k, ku) in enumerate(zip(images, keys, keysUn)):
        wu, wd, w_with, w_out = rr.compute_stereo_from_rgbd(im, factor, k, ku, rr.BF)
        print("frame %d: %d key points, %d with depth, %d outside" % (f, len(k), w_with, w_out))
        assert got[f][0].tobytes() == wu.tobytes() and got[f][1].tobytes() == wd.tobytes(), f
        assert pu[first[f]:first[f + 1]].tobytes() == wu.tobytes() and pd[first[f]:first[f + 1]].tobytes() == wd.tobytes()
        assert (n_with[f], n_out[f]) == (w_with, w_out) and w_with == int((got[f][1] > 0).sum())
        if f < len(sizes) and len(k) >= 63:
            assert SHARE_LO <= n_with[f] / len(k) <= SHARE_HI
    assert n_out[-1] == 8 and n_with[-1] == 10 and np.all(n_out[:-1] == 0)
    # the one-frame mirror with a context, and a second call on the handle with fewer frames
    one = ComputeStereoFromRGBD(images[2], keys[2], keysUn[2], rr.BF, factor, ctx=ctx)
    assert one[0].tobytes() == got[2][0].tobytes() and one[1].tobytes() == got[2][1].tobytes()
    a.from_keys(keys[2:3], keysUn[2:3], rr.BF, factor)  # (frame 0's image is the same generator image)
    (again,), _, _ = a.read()
    assert again[0].tobytes() == got[2][0].tobytes()
    a.close()


def test_gather_from_orb_equals_from_keys_and_restatement(ctx):
    """Two 640 x 480 frames, 1 000 features, TUM1's calibration: Frame::UndistortKeyPoints and the gather from the extractor's device buffers."""
    import torch
    W, H = 640, 480
    gray = np.stack([sr.pair(s, W, H, sr.FIXED_BANDS)[0] for s in (31, 32)])
    depth = np.stack([rr.depth_image(s, W, H, np.uint16) for s in (41, 42)])
    ext = ORBextractor(1000, 1.2, 8, 20, 7, W, H, max_frames=2, ctx=ctx)
    ext.upload(gray)
    ext.run()
    res = ext.read()
    a = RGBDAssociator(W, H, ext.cap, 2, ctx=ctx)
    a.upload_depth(depth)
    a.from_orb(ext, rr.K4, rr.DIST5, rr.BF, rr.FACTOR)
    got, n_with, n_out = a.read()
    pu, pd, first, _, _ = a.read_packed()
    ku_dev = a.read_keys_un()
    keys = [res[f][0] for f in range(2)]
    keysUn = [rr.undistort_keypoints(k, rr.K4, rr.DIST5) for k in keys]
    assert ku_dev.tobytes() == np.concatenate(keysUn).tobytes()
    ctx.sync()
    for f in range(2):
        wu, wd, w_with, w_out = rr.compute_stereo_from_rgbd(depth[f], rr.FACTOR, keys[f], keysUn[f], rr.BF)
        n = len(keys[f])
        print("frame %d: %d key points, %d with depth" % (f, n, w_with))
        assert n > 900 and got[f][0].tobytes() == wu.tobytes() and got[f][1].tobytes() == wd.tobytes()
        assert pu[first[f]:first[f + 1]].tobytes() == wu.tobytes() and pd[first[f]:first[f + 1]].tobytes() == wd.tobytes()
        assert n_with[f] == w_with and n_out[f] == 0 == w_out and SHARE_LO <= w_with / n <= SHARE_HI
        du, dd, dk, dn = a.device_frame(f)
        assert dn == n
        assert torch.as_tensor(_Dev(du, n), device="cuda").cpu().numpy().tobytes() == wu.tobytes()
        assert torch.as_tensor(_Dev(dd, n), device="cuda").cpu().numpy().tobytes() == wd.tobytes()
        assert torch.as_tensor(_Dev(dk, n * 7), device="cuda").cpu().numpy().tobytes() == keysUn[f].tobytes()
    # the second frame alone, and without distortion (mvKeysUn = mvKeys)
    a.from_orb(ext, rr.K4, rr.DIST5, rr.BF, rr.FACTOR, first_frame=1, n_frames=1)
    (one,), _, _ = a.read()
    wu1 = rr.compute_stereo_from_rgbd(depth[0], rr.FACTOR, keys[1], keysUn[1], rr.BF)[0]  # frame 1's key points over depth image 0
    assert one[0].tobytes() == wu1.tobytes()
    a.from_orb(ext, rr.K4, None, rr.BF, rr.FACTOR)
    plain, _, _ = a.read()
    assert plain[0][0].tobytes() == rr.compute_stereo_from_rgbd(depth[0], rr.FACTOR, keys[0], keys[0], rr.BF)[0].tobytes() != got[0][0].tobytes()
    # the same key points through from_keys
    b = RGBDAssociator(W, H, ext.cap, 2, ctx=ctx)
    b.upload_depth(depth)
    b.from_keys(keys, keysUn, rr.BF, rr.FACTOR)
    other, _, _ = b.read()
    assert all(other[f][0].tobytes() == got[f][0].tobytes() and other[f][1].tobytes() == got[f][1].tobytes() for f in range(2))
    # a depth batch that is already on the device
    t = torch.as_tensor(depth.view(np.int16)).cuda()
    b.set_depth_device(t.data_ptr(), np.uint16, 2)
    b.from_orb(ext, rr.K4, rr.DIST5, rr.BF, rr.FACTOR)
    dev, _, _ = b.read()
    assert all(dev[f][0].tobytes() == got[f][0].tobytes() for f in range(2))
    a.close(); b.close(); ext.close()


_CASES = {}


def _close_cases():
    """The frames of the close-point calls and what the restatement gives for them, computed once: per (shift of the need_new patterns, mode) a list of dicts."""
    if not _CASES:
        cases = rr.close_cases(CP_CAP)
        first = np.concatenate([[0], np.cumsum([len(z) for _, z in cases])]).astype(np.int32)
        T = rr.poses(len(cases))
        ku = rr.keypoints(77, first[-1], 640, 480)
        depth = np.concatenate([z for _, z in cases])
        needs = [np.concatenate([rr.need_new_pattern(f + shift, len(z)) for f, (_, z) in enumerate(cases)]) for shift in range(3)]
        want = {}
        for shift in range(3):
            for mode in (CS_CLOSE_POINTS_NEAREST, CS_CLOSE_POINTS_ALL):
                if mode == CS_CLOSE_POINTS_ALL and shift:
                    want[shift, mode] = want[0, mode]  # need_new is ignored
                    continue
                want[shift, mode] = [rr.close_points(z, ku[first[f]:first[f + 1]], needs[shift][first[f]:first[f + 1]], T[f], rr.K4, rr.TH_DEPTH, mode)
                                     for f, (_, z) in enumerate(cases)]
        _CASES.update(cases=cases, first=first, T=T, ku=ku, depth=depth, needs=needs, want=want)
    return _CASES


def _pixel_frames(depths, W, H):
    """One F32 image and one key point per depth value: key point i sits in pixel i, so that factor 1 hands the value over unchanged."""
    images, keys = np.zeros((len(depths), H, W), f32), []
    for f, z in enumerate(depths):
        images[f].flat[:len(z)] = z
        k = np.zeros(len(z), KEYPOINT_DTYPE)
        k["x"], k["y"] = np.arange(len(z)) % W + 0.25, np.arange(len(z)) // W + 0.5
        keys.append(k)
    return images, keys


def _check_call(c, got, shift, mode):
    partly = 0
    for f, (name, _) in enumerate(c["cases"]):
        want = c["want"][shift, mode][f]
        _same_close(got[f], want, (name, shift, mode))
        partly += 0 < len(want["new_idx"]) < want["n_valid"]
    if mode == CS_CLOSE_POINTS_NEAREST:
        assert partly >= 1
    else:  # every z > 0 in index order
        assert all(np.array_equal(got[f]["new_idx"], np.flatnonzero(z > 0)) and np.array_equal(got[f]["order"], got[f]["new_idx"]) for f, (_, z) in enumerate(c["cases"]))


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_close_points_host_arrays_equal_restatement(ctx, shift):
    """cs_close_points: n_valid over {0 .. 129, 1000, 2048} x c over {0, 99, 100, 101, n_valid}, equal / tie-heavy / threshold / +inf depths, need_new all 0, all 1 and
    alternating (which frame has which rotates with `shift`), every fourth pose not orthonormal."""
    c = _close_cases()
    for mode in (CS_CLOSE_POINTS_NEAREST, CS_CLOSE_POINTS_ALL):
        got = ClosePoints(c["depth"], c["ku"], c["needs"][shift], c["T"], rr.K4, rr.TH_DEPTH, mode, first=c["first"], ctx=ctx)
        _check_call(c, got, shift, mode)


def test_close_points_on_the_handle_equal_restatement(ctx):
    """cs_rgbd_close_points on what cs_rgbd_from_keys left on the device: the same frames, each depth value handed over through a pixel of an F32 image."""
    c = _close_cases()
    depths = [z for _, z in c["cases"]]
    images, keys = _pixel_frames(depths, CP_W, CP_H)
    a = RGBDAssociator(CP_W, CP_H, CP_CAP, len(depths), ctx=ctx)
    a.upload_depth(images)
    keysUn = [c["ku"][c["first"][f]:c["first"][f + 1]] for f in range(len(depths))]
    a.from_keys(keys, keysUn, rr.BF, 1.0)
    res, n_with, n_out = a.read()
    for f, z in enumerate(depths):
        assert res[f][1].tobytes() == np.where(z > 0, z, f32(-1)).astype(f32).tobytes() and n_with[f] == int((z > 0).sum()) and n_out[f] == 0
    for shift in range(3):
        for mode in (CS_CLOSE_POINTS_NEAREST, CS_CLOSE_POINTS_ALL):
            _check_call(c, a.close_points(c["needs"][shift] if mode == CS_CLOSE_POINTS_NEAREST or shift else None, c["T"], rr.K4, rr.TH_DEPTH, mode), shift, mode)
    a.close()


def test_close_points_special_thresholds_and_the_largest_frame(ctx):
    T = rr.poses(4)
    ku = rr.keypoints(5, CS_RGBD_MAX_KEYPOINTS, 640, 480)
    ones = np.ones(CS_RGBD_MAX_KEYPOINTS, np.uint8)
    # all depths equal and beyond the threshold: the first 101 by index
    z = np.ones(150, f32)
    r = ClosePoints(z, ku[:150], ones[:150], T[3], rr.K4, 0.5, ctx=ctx)
    _same_close(r, rr.close_points(z, ku[:150], ones[:150], T[3], rr.K4, 0.5, rr.NEAREST), "equal beyond")
    assert r["n_walked"] == 101 and np.array_equal(r["new_idx"], np.arange(101))
    # a NaN threshold is never exceeded: the walk takes every point
    r = ClosePoints(z, ku[:150], ones[:150], T[1], rr.K4, float("nan"), ctx=ctx)
    _same_close(r, rr.close_points(z, ku[:150], ones[:150], T[1], rr.K4, float("nan"), rr.NEAREST), "nan threshold")
    assert r["n_walked"] == 150
    # CS_RGBD_MAX_KEYPOINTS key points, all with depth, tie-heavy: the whole LDS sort, in both forms
    z = rr.close_case(9, CS_RGBD_MAX_KEYPOINTS + 2000, 5000, rr.TH_DEPTH, "u16")
    z = z[z > 0][:CS_RGBD_MAX_KEYPOINTS]
    need = rr.need_new_pattern(2, len(z))
    want = rr.close_points(z, ku, need, T[2], rr.K4, rr.TH_DEPTH, rr.NEAREST)
    assert want["n_valid"] == CS_RGBD_MAX_KEYPOINTS and 100 < want["n_walked"] < want["n_valid"] and 0 < len(want["new_idx"]) < want["n_walked"]
    _same_close(ClosePoints(z, ku, need, T[2], rr.K4, rr.TH_DEPTH, ctx=ctx), want, "largest, host arrays")
    images, keys = _pixel_frames([z], CP_W, CP_H)
    a = RGBDAssociator(CP_W, CP_H, CS_RGBD_MAX_KEYPOINTS, 1, ctx=ctx)
    a.upload_depth(images)
    a.from_keys(keys, [ku], rr.BF, 1.0)
    _same_close(a.close_points(need, T[2:3], rr.K4, rr.TH_DEPTH)[0], want, "largest, handle")
    # Tracking.UpdateLastFrame on the same handle: ids in creation order
    t = Tracking(ctx=ctx, sensor=Tracking.RGBD)
    mp = np.where(need != 0, -1, 0)
    slots, ids, x3D = t.UpdateLastFrame(None, None, mp, np.array([2]), T[2], rr.K4, rr.TH_DEPTH, next_point_id=50, rgbd=a)
    assert ids == list(range(50, 50 + len(want["new_idx"]))) == t.mlpTemporalPoints and np.array_equal(slots[want["new_idx"]], ids) and x3D.tobytes() == want["new_x3D"].tobytes()
    idx, pts = t.StereoInitializationPoints(z[:600], ku[:600], T[0], rr.K4)
    assert np.array_equal(idx, np.arange(600)) and pts.tobytes() == rr.close_points(z[:600], ku[:600], None, T[0], rr.K4, 0.0, rr.ALL)["new_x3D"].tobytes()
    t.close(); a.close()


def test_close_points_compaction_seams(ctx):
    """Both ordered compactions of rgbd_close_points (block_rank over the 16 waves of a pass of 1 024 threads) over tests/compaction_seams.py, and at the pass itself
    (1 023, 1 024, 1 025).  The first compaction's flag is z > 0: mode ALL with the pattern in the depths, where the second one takes every valid point.  The second
    one's flag is need_new over the walked prefix: equal depths under a NaN threshold, which is never exceeded, so the walk is every point in index order."""
    from tests import compaction_seams as cs
    cases = cs.cases(cs.SIZES + [1023, 1024, 1025])
    first = np.concatenate([[0], np.cumsum([n for n, _, _ in cases])]).astype(np.int32)
    T, ku = rr.poses(len(cases)), rr.keypoints(78, first[-1], 640, 480)
    flag = np.concatenate([fl for _, _, fl in cases])
    ones = np.ones(first[-1], f32)
    for mode, depth, need, th in ((CS_CLOSE_POINTS_ALL, np.where(flag, f32(1.5), f32(0)).astype(f32), None, rr.TH_DEPTH), (CS_CLOSE_POINTS_NEAREST, ones, flag.astype(np.uint8), float("nan"))):
        got = ClosePoints(depth, ku, need, T, rr.K4, th, mode, first=first, ctx=ctx)
        for f, (n, pattern, fl) in enumerate(cases):
            s = slice(first[f], first[f + 1])
            _same_close(got[f], rr.close_points(depth[s], ku[s], None if need is None else need[s], T[f], rr.K4, th, mode), (n, pattern, mode))
            assert np.array_equal(got[f]["new_idx"], np.flatnonzero(fl)) and got[f]["n_valid"] == (int(fl.sum()) if mode == CS_CLOSE_POINTS_ALL else n)


def test_errors(ctx):
    lib = _lib.lib()
    W, H = 640, 480
    pf = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    h = C.c_void_p()
    assert lib.cs_rgbd_create(ctx.ptr, W, H, CS_RGBD_MAX_KEYPOINTS + 1, 1, C.byref(h)) == BAD_ARG and not h.value
    assert b"CS_RGBD_MAX_KEYPOINTS" in lib.cs_last_error(ctx.ptr)
    assert lib.cs_rgbd_create(ctx.ptr, 0, H, 100, 1, C.byref(h)) == BAD_ARG and lib.cs_rgbd_create(ctx.ptr, W, H, 100, 0, C.byref(h)) == BAD_ARG
    ext = ORBextractor(1000, 1.2, 8, 20, 7, W, H, max_frames=2, ctx=ctx)
    ext.upload(np.stack([sr.pair(31, W, H, sr.FIXED_BANDS)[0]] * 2))
    ext.run()
    n = len(ext.read()[0][0])
    a = RGBDAssociator(W, H, ext.cap, 2, ctx=ctx)
    K, D = np.ascontiguousarray(rr.K4), np.ascontiguousarray(rr.DIST5)
    call = lambda h_, e, f0, nf, k4, bf: lib.cs_rgbd_from_orb(ctx.ptr, h_._h, e._e, f0, nf, None if k4 is None else pf(k4), pf(D), C.c_float(bf), C.c_float(rr.FACTOR))
    assert call(a, ext, 0, 1, K, rr.BF) == BAD_ARG  # no depth image yet
    depth = np.stack([rr.depth_image(s, W, H, np.uint16) for s in (41, 42)])
    a.upload_depth(depth)
    assert call(a, ext, 0, 2, K, rr.BF) == 0
    assert call(a, ext, 0, 3, K, rr.BF) == BAD_ARG   # beyond the run and the handle
    assert call(a, ext, 1, 2, K, rr.BF) == BAD_ARG   # beyond the run
    assert call(a, ext, 0, 0, K, rr.BF) == BAD_ARG and call(a, ext, -1, 1, K, rr.BF) == BAD_ARG
    assert call(a, ext, 0, 1, K, 0.0) == BAD_ARG and call(a, ext, 0, 1, K, -1.0) == BAD_ARG and call(a, ext, 0, 1, K, float("nan")) == BAD_ARG
    assert call(a, ext, 0, 1, None, rr.BF) == BAD_ARG
    a.upload_depth(depth[:1])
    assert call(a, ext, 0, 2, K, rr.BF) == BAD_ARG   # more frames than depth images
    fresh = ORBextractor(1000, 1.2, 8, 20, 7, W, H, ctx=ctx)  # no run yet
    assert call(a, fresh, 0, 1, K, rr.BF) == BAD_ARG
    other = ORBextractor(1000, 1.2, 8, 20, 7, 752, 480, ctx=ctx)
    other.upload(np.zeros((480, 752), np.uint8))
    other.run()
    assert call(a, other, 0, 1, K, rr.BF) == BAD_ARG  # the frame size differs from the depth images'
    assert lib.cs_rgbd_upload_depth(ctx.ptr, a._h, C.c_void_p(depth.ctypes.data), 2, 1, C.c_long(W * 2)) == BAD_ARG  # not a depth type
    assert lib.cs_rgbd_upload_depth(ctx.ptr, a._h, C.c_void_p(depth.ctypes.data), 0, 3, C.c_long(W * 2)) == BAD_ARG
    assert lib.cs_rgbd_upload_depth(ctx.ptr, a._h, C.c_void_p(depth.ctypes.data), 0, 1, C.c_long(W * 2 - 1)) == BAD_ARG
    # capacity: a handle one below the frame's count; a read with room for one fewer copies nothing
    small = RGBDAssociator(W, H, n - 1, 1, ctx=ctx)
    small.upload_depth(depth[:1])
    assert call(small, ext, 0, 1, K, rr.BF) == CAPACITY
    exact = RGBDAssociator(W, H, n, 1, ctx=ctx)
    exact.upload_depth(depth[:1])
    assert call(exact, ext, 0, 1, K, rr.BF) == 0
    u, d = np.full(n, 7, f32), np.full(n, 7, f32)
    cnt, nd = np.zeros(1, np.int32), np.zeros(1, np.int32)
    assert lib.cs_rgbd_read(ctx.ptr, exact._h, pf(u), pf(d), n - 1, pi(cnt), pi(nd), None) == CAPACITY and np.all(u == 7) and np.all(d == 7)
    first, total = np.zeros(2, np.int32), C.c_long()
    assert lib.cs_rgbd_read_packed(ctx.ptr, exact._h, pf(u), pf(d), C.c_long(n - 1), pi(first), C.byref(total), None, None) == CAPACITY and np.all(u == 7) and total.value == n
    assert lib.cs_rgbd_read(ctx.ptr, exact._h, pf(u), pf(d), n, pi(cnt), pi(nd), None) == 0 and cnt[0] == n and SHARE_LO * n <= nd[0] == int((d > 0).sum()) <= SHARE_HI * n
    p = [C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.c_void_p()]
    k = C.c_int()
    assert lib.cs_rgbd_device_frame(exact._h, 1, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(k)) == BAD_ARG
    assert lib.cs_rgbd_device_frame(exact._h, 0, C.byref(p[0]), C.byref(p[1]), None, C.byref(k)) == 0 and k.value == n
    # the close-point calls
    z, ku = np.ones(10, f32), rr.keypoints(1, 10, W, H)
    with pytest.raises(_lib.CubeSlamError, match="need_new"):
        ClosePoints(z, ku, None, rr.poses(1)[0], rr.K4, 1.0, ctx=ctx)
    with pytest.raises(_lib.CubeSlamError, match="mode"):
        ClosePoints(z, ku, np.ones(10, np.uint8), rr.poses(1)[0], rr.K4, 1.0, 2, ctx=ctx)
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_CAPACITY"):
        ClosePoints(np.ones(8193, f32), rr.keypoints(1, 8193, W, H), np.ones(8193, np.uint8), rr.poses(1)[0], rr.K4, 1.0, ctx=ctx)
    exact.from_orb(ext, rr.K4, rr.DIST5, rr.BF, rr.FACTOR, n_frames=1)
    with pytest.raises(_lib.CubeSlamError, match="need_new"):
        exact.close_points(None, rr.poses(1), rr.K4, 1.0)
    assert exact.close_points(None, rr.poses(1), rr.K4, 1.0, CS_CLOSE_POINTS_ALL)[0]["n_valid"] == nd[0]
    for x in (a, small, exact, fresh, other, ext):
        x.close()
