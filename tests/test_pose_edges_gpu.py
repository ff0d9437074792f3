"""GPU parity of PoseOptimization (pose_opt_kernel, cs_pose_optimization) at the sizes where its 256-thread stride and its 64-lane / four-wave reduction have seams, on the
paths of the routine that ordinary frames do not reach, under more than one camera, and in a batch of unlike neighbours -- against the oracle's orc_pose_optimization
(pinned to the reference's own text by tests/test_ref_graph_pins.py).  The cases are tests/pose_patterns.py's; tests/test_pose_patterns.py shows from the oracle alone that
no chi2 of theirs sits on a threshold and that no decision of theirs flips under reordering, so flags and counts must be equal and the pose must agree within
P.TOL = 100 x D_REF, the oracle's own sensitivity to the order of its edges.

Observed on an MI355X (largest device-to-oracle pose difference; P.TOL = 2.1e-12): 2.5e-14 over the sizes (n3), 4.1e-14 over the path cases (one_point), 4.4e-16 over the
camera cases; flags and counts equal everywhere."""
import ctypes as C

import numpy as np
import pytest

from cube_slam_amd import _lib
from cube_slam_amd.optimizer import PoseOptimization
from tests import pose_patterns as P

pytestmark = pytest.mark.gpu

BAD_ARG = -2  # CS_ERR_BAD_ARG


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def _check(oracle, name, got):
    pose, flags, n_in = got
    wpose, wflags, wn, _ = P.judged(oracle, name)
    d = P.pose_distance(pose, wpose)
    print("%s: n_inliers %d / %d, flags differing %d of %d, pose distance %.3e (TOL %.3e)" % (name, n_in, wn, int((flags != wflags).sum()), len(wflags), d, P.TOL))
    assert np.all(np.isfinite(pose))
    assert n_in == wn
    assert flags.tobytes() == wflags.tobytes()
    assert d <= P.TOL


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_alone_equals_the_oracle(ctx, oracle, name):
    fr = P.case(name)
    got = PoseOptimization([fr], ctx=ctx)
    assert len(got) == 1
    pose, flags, n_in = got[0]
    _check(oracle, name, got[0])
    start = P.normalised(fr["pose"])
    if name == "all_outliers":
        assert n_in == 0 and flags.all() and pose.tobytes() == start.tobytes()
    if name == "zero_weights":
        assert n_in == len(flags) and not flags.any() and pose.tobytes() == start.tobytes()
    if name in ("n0", "n2"):
        assert n_in == 0 and not flags.any() and pose.tobytes() == start.tobytes()
    if name == "far_start":
        assert np.linalg.norm(pose[:3] - fr["pose_true"][:3]) < 1e-3 < 7.99 < np.linalg.norm(fr["pose"][:3] - fr["pose_true"][:3])
    if name == "quat_unnormalised":
        assert pose[6] > 0 and abs(np.linalg.norm(pose[3:]) - 1) < 1e-15


@pytest.mark.parametrize("a, b", [("cam_kitti", "cam_tum"), ("bf_a", "bf_b")])
def test_the_camera_is_the_frames_own(ctx, oracle, a, b):
    """One geometry under two cameras, one stereo frame under two rigs: alone and side by side, either order, each frame gets the pose of its own camera."""
    alone = [PoseOptimization([P.case(k)], ctx=ctx)[0] for k in (a, b)]
    assert P.pose_distance(alone[0][0], alone[1][0]) > 1e-4  # a thousand times what the two could differ by if the camera did not matter
    pair, riap = PoseOptimization([P.case(a), P.case(b)], ctx=ctx), PoseOptimization([P.case(b), P.case(a)], ctx=ctx)[::-1]
    for k, x, p, r in zip((a, b), alone, pair, riap):
        assert _same(x, p) and _same(x, r), k
        _check(oracle, k, p)


def test_a_batch_equals_its_frames_alone_and_itself(ctx, oracle):
    frames = [P.case(k) for k in P.BATCH]
    batch = PoseOptimization(frames, ctx=ctx)
    again = PoseOptimization(frames, ctx=ctx)
    back = PoseOptimization(frames[::-1], ctx=ctx)[::-1]  # a frame's result does not depend on its place or its neighbours
    assert len(batch) == len(P.BATCH)
    for k, b, a, r in zip(P.BATCH, batch, again, back):
        s = PoseOptimization([P.case(k)], ctx=ctx)[0]
        assert _same(b, s), k
        assert _same(b, a), k
        assert _same(b, r), k
        _check(oracle, k, b)


def test_bad_arguments_are_refused_before_the_device(ctx):
    """Through the C entry itself: each refusal returns CS_ERR_BAD_ARG and leaves pose_out, outlier and n_inliers as they were."""
    f = _lib.lib().cs_pose_optimization
    frames = [P.case("n11"), P.case("n4")]
    off = np.array([0, 11, 15], np.int32)
    Xw = np.ascontiguousarray(np.concatenate([fr["Xw"] for fr in frames]))
    obs = np.ascontiguousarray(np.concatenate([fr["obs"] for fr in frames]))
    w = np.ascontiguousarray(np.concatenate([fr["inv_sigma2"] for fr in frames]))
    intr = np.ascontiguousarray(np.stack([fr["intr"] for fr in frames]))
    pin = np.ascontiguousarray(np.stack([fr["pose"] for fr in frames]))
    pout, flags, ninl = np.full((2, 7), 77.0), np.full(15, 7, np.uint8), np.full(2, -7, np.int32)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    good = {"n_frames": 2, "edge_off": off.ctypes.data_as(C.POINTER(C.c_int)), "Xw": dp(Xw), "obs": dp(obs), "inv_sigma2": dp(w), "intrinsics": dp(intr), "pose_in": dp(pin),
            "pose_out": dp(pout), "outlier": flags.ctypes.data_as(C.POINTER(C.c_uint8)), "n_inliers": ninl.ctypes.data_as(C.POINTER(C.c_int))}

    def call(**kw):
        a = dict(good, **kw)
        return f(ctx.ptr, a["n_frames"], a["edge_off"], a["Xw"], a["obs"], a["inv_sigma2"], a["intrinsics"], a["pose_in"], a["pose_out"], a["outlier"], a["n_inliers"])

    def untouched():
        return np.all(pout == 77.0) and np.all(flags == 7) and np.all(ninl == -7)

    for dec in ([0, 11, 10], [0, 15, 0], [5, 3, 15]):
        d = np.array(dec, np.int32)
        assert call(edge_off=d.ctypes.data_as(C.POINTER(C.c_int))) == BAD_ARG and untouched(), dec
    for k in ("Xw", "obs", "inv_sigma2", "outlier", "pose_in", "pose_out", "n_inliers", "edge_off", "intrinsics"):
        assert call(**{k: None}) == BAD_ARG and untouched(), k
    assert call(n_frames=-1) == BAD_ARG and untouched()
    assert f(None, *[good[k] for k in good]) == BAD_ARG and untouched()
    assert call(n_frames=0) == _lib.CS_OK and untouched()
    assert call(n_frames=0, Xw=None, obs=None, inv_sigma2=None, intrinsics=None, pose_in=None, pose_out=None, outlier=None, n_inliers=None) == _lib.CS_OK
    assert PoseOptimization([], ctx=ctx) == []
    # and the arrays are good ones: the same call goes through and writes all three results
    assert call() == _lib.CS_OK and not np.any(pout == 77.0) and np.all(flags <= 1) and np.all(ninl >= 0)
    for i, fr in enumerate(frames):
        assert _same((pout[i], flags[off[i]:off[i + 1]], int(ninl[i])), PoseOptimization([fr], ctx=ctx)[0])
