"""CPU: what tests/rgbd_restatement.py states, pinned: the walk's closed form against the reference's loop, the special depth values, and the shares of key points with
depth / of created points for every generator the GPU tests use (the floors and bands of tests/test_rgbd_gpu.py are read from these prints)."""
import numpy as np

from tests import rgbd_restatement as rr

f32 = np.float32


def test_closed_form_equals_the_loop():
    """n_valid 0 .. 260, c 0 .. n_valid: sorted depths of which the first c are not beyond the threshold."""
    th = 3.0
    for n in range(261):
        for c in range(n + 1):
            z = [1.0] * c + [4.0] * (n - c)
            assert rr.walk(z, th) == rr.closed_form(n, c), (n, c)
    # a depth equal to the threshold is not beyond it; +inf is; a NaN threshold is never exceeded
    assert rr.walk([3.0] * 150, 3.0) == 150 and rr.walk([3.0] * 100 + [np.inf] * 50, 3.0) == 101
    assert rr.walk([1.0] * 150, float("nan")) == 150 == rr.closed_form(150, 150)


def test_special_samples():
    assert rr.FACTOR == float(f32(0.0002)) and rr.convert_sample(np.uint16(65535), rr.FACTOR) == f32(f32(65535.0) * f32(0.0002))
    assert rr.convert_sample(np.uint16(65535), 1.0) == f32(65535.0) and rr.convert_sample(f32(1.25), 1.0) == f32(1.25)  # factor 1 is the exact copy
    k = rr.keypoints(1, 5, 8, 8)
    k["x"], k["y"] = [0, 1, 2, 3, 4], 0
    ku = k.copy()
    ku["x"] += f32(0.5)
    im = np.zeros((8, 8), f32)
    im[0, :5] = [np.nan, np.inf, 0.0, -2.0, 2.0]
    ur, d, n_with, n_out = rr.compute_stereo_from_rgbd(im, 1.0, k, ku, 40.0)
    assert n_with == 2 and n_out == 0
    assert np.array_equal(d, np.array([-1, np.inf, -1, -1, 2], f32)) and np.array_equal(ur, np.array([-1, 1.5, -1, -1, f32(4.5) - f32(40.0) / f32(2.0)], f32))
    # truncation toward zero: (-1, 0) is column 0; W - 1 + 0.999 is the last column; W is outside; NaN is outside
    e = rr.edge_keypoints(64, 48)
    for dt in (np.uint16, np.float32):
        ur, d, n_with, n_out = rr.compute_stereo_from_rgbd(rr.edge_image(64, 48, dt), 1.0, e, e, 40.0)
        assert n_out == 8 and np.all(d[[5, 8, 9, 10, 11, 12, 13, 14]] == -1) and np.all(d[[0, 1, 2, 3, 4, 6, 7]] > 0)
        assert np.array_equal(d[15:], np.array([-1, -1, 65535, 1, 65535] if dt == np.uint16 else [-1, -1, np.inf, 1, 65535], f32))
        assert n_with == int((d > 0).sum()) == 10


def test_pose_matrices_and_unprojection():
    T = rr.poses(4)
    for f in range(4):
        Rwc, Ow = rr.update_pose_matrices(T[f])
        assert np.array_equal(Rwc, T[f, :, :3].T) and np.allclose(Ow, -(T[f, :, :3].astype(np.float64).T @ T[f, :, 3].astype(np.float64)), rtol=1e-6)
    Rwc, Ow = rr.update_pose_matrices(np.eye(4, dtype=f32)[:3])
    x = rr.unproject_stereo(rr.K4[2] + f32(10), rr.K4[3] - f32(20), 2.0, rr.K4, Rwc, Ow)
    assert np.allclose(x, [20 / rr.K4[0], -40 / rr.K4[1], 2.0], rtol=1e-6)
    # z = +inf: 0 * inf in the product with the identity; the NaN of an invalid operation is the host's default NaN (sign set on x86, where the reference runs)
    x = rr.unproject_stereo(400.0, 100.0, np.inf, rr.K4, Rwc, Ow)
    assert np.all(np.isnan(x)) and x.view(np.uint32).tolist() == [0xFFC00000] * 3


def test_undistortion_moves_the_key_points():
    """With TUM1's coefficients mvKeysUn differs from mvKeys by more than a pixel at the border, so a mix-up of the two shows in mvuRight (x of mvKeysUn) and in the sample
    (row / column of mvKeys)."""
    k = rr.keypoints(2, 300, 640, 480)
    ku = rr.undistort_keypoints(k, rr.K4, rr.DIST5)
    moved = np.hypot(ku["x"] - k["x"], ku["y"] - k["y"])
    assert moved.max() > 5 and (moved > 0.5).mean() > 0.5
    assert rr.undistort_keypoints(k, rr.K4, None).tobytes() == k.tobytes() and np.array_equal(ku["angle"], k["angle"])


def test_generator_shares():
    """The shares the GPU tests assert on, from the restatement alone."""
    W, H = 64, 48
    K = rr.small_K4(W, H)
    lo, hi = 1.0, 0.0
    for dt, factor in ((np.uint16, rr.FACTOR), (np.float32, 1.0)):
        im = rr.depth_image(3, W, H, dt)
        for n in rr.FRAME_SIZES:
            k = rr.keypoints(n + 5, n, W, H)
            _, d, n_with, n_out = rr.compute_stereo_from_rgbd(im, factor, k, rr.undistort_keypoints(k, K, rr.DIST5), rr.BF)
            print("gather %s n=%d share with depth %.3f outside %d" % (dt.__name__, n, n_with / max(n, 1), n_out))
            if n >= 63:
                lo, hi = min(lo, n_with / n), max(hi, n_with / n)
    print("full frames: %.3f - %.3f" % (lo, hi))
    assert 0.70 <= lo and hi <= 0.88  # tests/test_rgbd_gpu.py asserts this band widened by 0.1 on either side
    cases = rr.close_cases(1500)
    T = rr.poses(len(cases))
    partly = 0
    for f, (name, z) in enumerate(cases):
        r = rr.close_points(z, rr.keypoints(100 + f, len(z), 640, 480), rr.need_new_pattern(f, len(z)), T[f], rr.K4, rr.TH_DEPTH, rr.NEAREST)
        print("close %s n_valid=%d walked=%d created=%d" % (name, r["n_valid"], r["n_walked"], len(r["new_idx"])))
        partly += 0 < len(r["new_idx"]) < r["n_valid"]
    assert partly >= 10
