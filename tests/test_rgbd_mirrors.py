"""CPU: the Python mirrors of the RGB-D frame and of the close-point rule on their path without a context (ComputeStereoFromRGBD / ClosePoints with ctx=None, the
library's host statement over csrc/rgbd_math.h) against tests/rgbd_restatement.py, byte for byte; Tracking.UpdateLastFrame / StereoInitializationPoints over them."""
import numpy as np
import pytest

from cube_slam_amd import ClosePoints, ComputeStereoFromRGBD, Tracking
from cube_slam_amd.rgbd import CS_CLOSE_POINTS_ALL, CS_CLOSE_POINTS_NEAREST
from tests import rgbd_restatement as rr

f32 = np.float32


def _same_close(got, want, what):
    assert got["n_valid"] == want["n_valid"] and got["n_walked"] == want["n_walked"], what
    for key in ("order", "new_idx", "new_x3D"):
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (what, key)


@pytest.mark.parametrize("dt,factor", [(np.uint16, rr.FACTOR), (np.float32, 1.0), (np.float32, 0.5)])
def test_gather_equals_restatement(dt, factor):
    W, H = 64, 48
    K = rr.small_K4(W, H)
    frames = [(rr.depth_image(3, W, H, dt), rr.keypoints(n + 5, n, W, H)) for n in rr.FRAME_SIZES] + [(rr.edge_image(W, H, dt), rr.edge_keypoints(W, H))]
    for im, k in frames:
        ku = rr.undistort_keypoints(k, K, rr.DIST5)
        wu, wd, n_with, n_out = rr.compute_stereo_from_rgbd(im, factor, k, ku, rr.BF)
        gu, gd, counts = ComputeStereoFromRGBD(im, k, ku, rr.BF, factor, counts=True)
        assert gu.tobytes() == wu.tobytes() and gd.tobytes() == wd.tobytes() and counts == (n_with, n_out), len(k)
        if len(k):  # a caller that hands mvKeys over twice gets another answer: the inputs tell the two apart
            assert ComputeStereoFromRGBD(im, k, k, rr.BF, factor)[0].tobytes() != wu.tobytes()


def test_gather_reads_a_strided_image():
    wide = np.zeros((48, 100), np.uint16)
    wide[:, :64] = rr.depth_image(4, 64, 48, np.uint16)
    wide[:, 64:] = 12345
    k = rr.keypoints(9, 200, 64, 48)
    want = ComputeStereoFromRGBD(np.ascontiguousarray(wide[:, :64]), k, k, rr.BF, rr.FACTOR)
    got = ComputeStereoFromRGBD(wide[:, :64], k, k, rr.BF, rr.FACTOR)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and 0.6 < (got[1] > 0).mean() < 0.9


def test_close_points_equal_restatement():
    cases = rr.close_cases(1500)
    T = rr.poses(len(cases))
    first = np.concatenate([[0], np.cumsum([len(z) for _, z in cases])]).astype(np.int32)
    ku = rr.keypoints(77, first[-1], 640, 480)
    depth = np.concatenate([z for _, z in cases])
    for shift in range(3):
        need = np.concatenate([rr.need_new_pattern(f + shift, len(z)) for f, (_, z) in enumerate(cases)])
        for mode in (CS_CLOSE_POINTS_NEAREST, CS_CLOSE_POINTS_ALL):
            batch = ClosePoints(depth, ku, need, T, rr.K4, rr.TH_DEPTH, mode, first=first)
            partly = 0
            for f, (name, z) in enumerate(cases):
                s = slice(first[f], first[f + 1])
                want = rr.close_points(z, ku[s], need[s], T[f], rr.K4, rr.TH_DEPTH, mode)
                _same_close(batch[f], want, (name, shift, mode))
                partly += 0 < len(want["new_idx"]) < want["n_valid"]
                if shift == 0:
                    _same_close(ClosePoints(z, ku[s], need[s], T[f], rr.K4, rr.TH_DEPTH, mode), want, name)
            assert partly >= 1 or mode == CS_CLOSE_POINTS_ALL
    z = np.ones(150, f32)  # all depths equal and beyond the threshold: the first 101 by index
    r = ClosePoints(z, ku[:150], np.ones(150, np.uint8), T[3], rr.K4, 0.5)
    _same_close(r, rr.close_points(z, ku[:150], np.ones(150, np.uint8), T[3], rr.K4, 0.5, rr.NEAREST), "equal beyond")
    assert r["n_walked"] == 101 and np.array_equal(r["new_idx"], np.arange(101))


def test_close_points_arguments():
    from cube_slam_amd import _lib
    ku = rr.keypoints(1, 10, 640, 480)
    z = np.ones(10, f32)
    with pytest.raises(_lib.CubeSlamError):
        ClosePoints(z, ku, None, rr.poses(1)[0], rr.K4, 1.0, CS_CLOSE_POINTS_NEAREST)  # the walk needs need_new
    with pytest.raises(_lib.CubeSlamError):
        ClosePoints(z, ku, np.ones(10, np.uint8), rr.poses(1)[0], rr.K4, 1.0, 2)
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_CAPACITY"):
        ClosePoints(np.ones(8193, f32), rr.keypoints(1, 8193, 640, 480), np.ones(8193, np.uint8), rr.poses(1)[0], rr.K4, 1.0)
    assert ClosePoints(z, ku, None, rr.poses(1)[0], rr.K4, 1.0, CS_CLOSE_POINTS_ALL)["n_valid"] == 10


def test_tracking_update_last_frame_and_stereo_initialization():
    """Tracking.UpdateLastFrame over index tables: the created points take the next map-point ids in creation order, enter mlpTemporalPoints in that order and fill the
    frame's slots; slots that hold a point with observations are left alone."""
    z = rr.close_case(5, 300, 180, rr.TH_DEPTH)
    n = len(z)
    ku = rr.keypoints(6, n, 640, 480)
    rng = np.random.default_rng(8)
    mvpMapPoints = np.where(rng.random(n) < 0.5, rng.integers(0, 50, n), -1).astype(np.int64)
    observations = rng.integers(0, 3, 50)
    Tcw = rr.poses(2)[1]
    need = np.array([p < 0 or observations[p] < 1 for p in mvpMapPoints], np.uint8)
    want = rr.close_points(z, ku, need, Tcw, rr.K4, rr.TH_DEPTH, rr.NEAREST)
    t = object.__new__(Tracking)  # (the constructor opens a device; these two methods need none with host=True)
    t.mSensor = Tracking.RGBD
    slots, temporal, x3D = t.UpdateLastFrame(z, ku, mvpMapPoints, observations, Tcw, rr.K4, rr.TH_DEPTH, next_point_id=1000, host=True)
    k = len(want["new_idx"])
    assert 0 < k < want["n_valid"] and temporal == list(range(1000, 1000 + k)) and t.mlpTemporalPoints == temporal
    assert np.array_equal(slots[want["new_idx"]], np.arange(1000, 1000 + k)) and x3D.tobytes() == want["new_x3D"].tobytes()
    untouched = np.setdiff1d(np.arange(n), want["new_idx"])
    assert np.array_equal(slots[untouched], mvpMapPoints[untouched])
    # monocular, or the last frame is the last key frame (Tracking.cc:1215): nothing is created
    assert t.UpdateLastFrame(z, ku, mvpMapPoints, observations, Tcw, rr.K4, rr.TH_DEPTH, next_point_id=0, last_frame_is_keyframe=True, host=True)[1] == []
    t.mSensor = Tracking.MONOCULAR
    assert t.UpdateLastFrame(z, ku, mvpMapPoints, observations, Tcw, rr.K4, rr.TH_DEPTH, next_point_id=0, host=True)[1] == []
    # StereoInitialization: N > 500 stays the caller's; every z > 0 in index order
    idx, pts = t.StereoInitializationPoints(z, ku, Tcw, rr.K4, host=True)
    want = rr.close_points(z, ku, None, Tcw, rr.K4, rr.TH_DEPTH, rr.ALL)
    assert np.array_equal(idx, np.flatnonzero(z > 0)) and pts.tobytes() == want["new_x3D"].tobytes()


def test_cpp_mirror_without_the_library(tmp_path):
    """tests/cpp/rgbd_mirror.cpp built with -DCUBESLAM_HOST_ONLY (nothing of the library), plain and a second time with the sanitizers, each run as a child process:
    byte-equal to the Python mirror on its host path and to the restatement."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-DCUBESLAM_HOST_ONLY", "-I", root, os.path.join(root, "tests", "cpp", "rgbd_mirror.cpp")]
    subprocess.check_call(base + ["-O2", "-o", str(tmp_path / "mirror")])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(tmp_path / "mirror_san")])
    frames = rr.mirror_frames()
    rr.write_mirror_input(tmp_path / "in.bin", frames)
    for exe in ("mirror", "mirror_san"):
        subprocess.check_call([str(tmp_path / exe), str(tmp_path / "in.bin"), str(tmp_path / (exe + ".out")), "host"], timeout=120)
        res = rr.read_mirror_output(tmp_path / (exe + ".out"), frames)
        some = 0
        for fr, (ur, dep, counts, r, again) in zip(frames, res):
            pu, pd, pc = ComputeStereoFromRGBD(fr["image"], fr["keys"], fr["keysUn"], fr["bf"], fr["factor"], counts=True)
            wu, wd, w_with, w_out = rr.compute_stereo_from_rgbd(fr["image"], fr["factor"], fr["keys"], fr["keysUn"], fr["bf"])
            assert ur.tobytes() == pu.tobytes() == wu.tobytes() and dep.tobytes() == pd.tobytes() == wd.tobytes() and counts == pc == (w_with, w_out)
            _same_close(r, ClosePoints(pd, fr["keysUn"], fr["need_new"], fr["Tcw"], fr["K4"], fr["th"], fr["mode"]), exe)
            _same_close(r, rr.close_points(wd, fr["keysUn"], fr["need_new"], fr["Tcw"], fr["K4"], fr["th"], fr["mode"]), exe)
            assert again.tobytes() == r["new_x3D"].tobytes()
            some += 0 < len(r["new_idx"]) < r["n_valid"]
        assert some >= 2
    assert subprocess.call([str(tmp_path / "mirror"), str(tmp_path / "in.bin"), str(tmp_path / "x.out")], stderr=subprocess.DEVNULL) == 2  # no device path in this build
