"""Python host-side mirror of ORB_SLAM2::Optimizer (reference orb_object_slam/include/Optimizer.h:36-52): PoseOptimization and OptimizeSim3 here,
BundleAdjustment / LocalBACameraPointObjects in cube_slam_amd.ba."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def PoseOptimization(frames, ctx=None, device=0):
    """frames: list of dicts {Xw (n,3), obs (n,3: u, v, u_right or -1), inv_sigma2 (n,), intr (fx, fy, cx, cy, bf), pose (7,)}.
    Returns a list of (pose (7,), outlier flags (n,) u8, n_inliers), one per frame -- what Optimizer::PoseOptimization(Frame*)
    writes into pFrame->mTcw / mvbOutlier and returns (Optimizer.cc:253-472)."""
    ctx = ctx or _lib.Context(device)
    F = len(frames)
    off = np.zeros(F + 1, np.int32)
    for f, fr in enumerate(frames):
        off[f + 1] = off[f] + len(fr["Xw"])
    ne = int(off[F])
    cat = lambda k, w: (np.concatenate([np.asarray(fr[k], np.float64).reshape(-1, w) for fr in frames]) if ne else np.zeros((1, w)))
    Xw, obs = np.ascontiguousarray(cat("Xw", 3)), np.ascontiguousarray(cat("obs", 3))
    w = np.ascontiguousarray(np.concatenate([np.asarray(fr["inv_sigma2"], np.float64).reshape(-1) for fr in frames])) if ne else np.zeros(1)
    intr = np.ascontiguousarray(np.stack([np.asarray(fr["intr"], np.float64) for fr in frames])) if F else np.zeros((1, 5))
    pin = np.ascontiguousarray(np.stack([np.asarray(fr["pose"], np.float64) for fr in frames])) if F else np.zeros((1, 7))
    pout = np.zeros((max(F, 1), 7)); flags = np.zeros(max(ne, 1), np.uint8); ninl = np.zeros(max(F, 1), np.int32)
    check(ctx.ptr, lib().cs_pose_optimization(ctx.ptr, F, _p(off, C.c_int), _p(Xw, C.c_double), _p(obs, C.c_double), _p(w, C.c_double), _p(intr, C.c_double),
                                              _p(pin, C.c_double), _p(pout, C.c_double), _p(flags, C.c_uint8), _p(ninl, C.c_int)), "cs_pose_optimization")
    return [(pout[f].copy(), flags[off[f]:off[f + 1]].copy(), int(ninl[f])) for f in range(F)]


def OptimizeSim3(problems, ctx=None, device=0):
    """Optimizer::OptimizeSim3 (Optimizer.cc:2838-3033) for one problem (a dict) or a batch (a list of dicts)
    {P1c (n,3), P2c (n,3), obs1 (n,2), obs2 (n,2), inv_sigma2_1 (n,), inv_sigma2_2 (n,), intrinsics (fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2), sim3_in (tx ty tz qx qy qz qw s),
    th2, fix_scale} over the correspondences that survive the reference's filter (:2893-2928), P1c / P2c being its float R * P + t products.
    Returns (sim3_out (8,), removed (n,) u8, n_inliers) per problem: g2oS12 as the reference leaves it (sim3_in bit for bit where it returns 0 before writing it),
    1 where it sets vpMatches1[idx] = NULL, and its return value.  A single dict gives a single tuple."""
    single = isinstance(problems, dict)
    if single:
        problems = [problems]
    ctx = ctx or _lib.Context(device)
    F = len(problems)
    if F == 0:
        return []
    off = np.zeros(F + 1, np.int32)
    for f, pr in enumerate(problems):
        off[f + 1] = off[f] + len(np.asarray(pr["inv_sigma2_1"]).reshape(-1))
    ne = int(off[F])
    cat = lambda k, w: np.ascontiguousarray(np.concatenate([np.asarray(pr[k], np.float64).reshape(-1, w) for pr in problems]) if ne else np.zeros((1, w)))
    P1, P2, o1, o2, w1, w2 = cat("P1c", 3), cat("P2c", 3), cat("obs1", 2), cat("obs2", 2), cat("inv_sigma2_1", 1), cat("inv_sigma2_2", 1)
    for a, w in ((P1, 3), (P2, 3), (o1, 2), (o2, 2), (w1, 1), (w2, 1)):
        if a.shape != (max(ne, 1), w):
            raise ValueError("OptimizeSim3: the arrays of a problem do not have one row per correspondence")
    intr = np.ascontiguousarray(np.stack([np.asarray(pr["intrinsics"], np.float64).reshape(8) for pr in problems]))
    sin = np.ascontiguousarray(np.stack([np.asarray(pr["sim3_in"], np.float64).reshape(8) for pr in problems]))
    th2 = np.ascontiguousarray([pr["th2"] for pr in problems], np.float32)
    fix = np.ascontiguousarray([1 if pr["fix_scale"] else 0 for pr in problems], np.uint8)
    sout = np.zeros((F, 8)); flags = np.zeros(max(ne, 1), np.uint8); ninl = np.zeros(F, np.int32)
    check(ctx.ptr, lib().cs_sim3_optimization(ctx.ptr, F, _p(off, C.c_int), _p(P1, C.c_double), _p(P2, C.c_double), _p(o1, C.c_double), _p(o2, C.c_double), _p(w1, C.c_double),
                                              _p(w2, C.c_double), _p(intr, C.c_double), _p(sin, C.c_double), _p(th2, C.c_float), _p(fix, C.c_uint8), _p(sout, C.c_double),
                                              _p(flags, C.c_uint8), _p(ninl, C.c_int)), "cs_sim3_optimization")
    res = [(sout[f].copy(), flags[off[f]:off[f + 1]].copy(), int(ninl[f])) for f in range(F)]
    return res[0] if single else res


def cuboid9_oplus(cub, upd, ctx=None, device=0):
    """g2o::VertexCuboid::oplusImpl for a batch (object_slam/include/object_slam/g2o_Object.h:193-204); cuboid = [t, q, half scale]."""
    ctx = ctx or _lib.Context(device)
    cub = np.ascontiguousarray(cub, np.float64).reshape(-1, 10); upd = np.ascontiguousarray(upd, np.float64).reshape(-1, 9)
    out = np.zeros_like(cub)
    check(ctx.ptr, lib().cs_cuboid9_oplus(ctx.ptr, len(cub), _p(cub, C.c_double), _p(upd, C.c_double), _p(out, C.c_double)), "cs_cuboid9_oplus")
    return out


def cuboid9_edge_linearize(cam_Tcw, cub_global, cub_meas, jac=True, ctx=None, device=0):
    """g2o::EdgeSE3Cuboid::computeError (+ g2o's numeric Jacobians) for a batch of camera-object edges (g2o_Object.h:227-252)."""
    ctx = ctx or _lib.Context(device)
    T = np.ascontiguousarray(cam_Tcw, np.float64).reshape(-1, 7); g = np.ascontiguousarray(cub_global, np.float64).reshape(-1, 10)
    m = np.ascontiguousarray(cub_meas, np.float64).reshape(-1, 10)
    n = len(T)
    err = np.zeros((n, 9)); Jc = np.zeros((n, 9, 6)); Jq = np.zeros((n, 9, 9))
    check(ctx.ptr, lib().cs_cuboid9_edge_linearize(ctx.ptr, n, _p(T, C.c_double), _p(g, C.c_double), _p(m, C.c_double), _p(err, C.c_double),
                                                   _p(Jc, C.c_double) if jac else None, _p(Jq, C.c_double) if jac else None), "cs_cuboid9_edge_linearize")
    return (err, Jc, Jq) if jac else err
