"""Python host-side mirror of ORB_SLAM2::Optimizer (reference orb_object_slam/include/Optimizer.h:36-52): PoseOptimization, OptimizeSim3 and OptimizeEssentialGraph here,
BundleAdjustment / LocalBACameraPointObjects in cube_slam_amd.ba."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Handle, check, lib, ptr


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
    check(ctx.ptr, lib().cs_pose_optimization(ctx.ptr, F, ptr(off), ptr(Xw), ptr(obs), ptr(w), ptr(intr),
                                              ptr(pin), ptr(pout), ptr(flags), ptr(ninl)), "cs_pose_optimization")
    return [(pout[f].copy(), flags[off[f]:off[f + 1]].copy(), int(ninl[f])) for f in range(F)]


def OptimizeSim3(problems, ctx=None, device=0):
    """Optimizer::OptimizeSim3 (Optimizer.cc:2838-3033) for one problem (a dict) or a batch (a list of dicts)
    {P1c (n,3), P2c (n,3), obs1 (n,2), obs2 (n,2), inv_sigma2_1 (n,), inv_sigma2_2 (n,), intrinsics (fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2), sim3_in (tx ty tz qx qy qz qw s),
    th2, fix_scale} over the correspondences that survive the reference's filter (:2893-2928), P1c / P2c being its float R * P + t products.
    Returns (sim3_out (8,), removed (n,) u8, n_inliers) per problem: g2oS12 as the reference leaves it (sim3_in bit for bit where it returns 0 before writing it),
    1 where it sets vpMatches1[idx] = NULL, and its return value.  A single dict gives a single tuple."""
    return _optimize_sim3(problems, ctx, device, None)


def OptimizeSim3Trace(problems, max_trials=150, ctx=None, device=0):
    """cs_sim3_optimization_trace (include/cubeslam_hip/sim3_opt_trace.h), a test probe: OptimizeSim3 through the same kernel, which also stores one record per
    Levenberg-Marquardt trial.  Returns (sim3_out, removed, n_inliers, trace (min(n_trials, max_trials), 7), n_trials, system0 (36,)) per problem; a trace row is
    stage, iteration, currentChi before, tempChi as computed, lambda used, solved, accepted; system0 is the lower triangle of H, b and chi2 of the first linearisation."""
    return _optimize_sim3(problems, ctx, device, int(max_trials))


def _optimize_sim3(problems, ctx, device, max_trials):
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
    args = (ctx.ptr, F, ptr(off), ptr(P1), ptr(P2), ptr(o1), ptr(o2), ptr(w1), ptr(w2), ptr(intr), ptr(sin), ptr(th2), ptr(fix), ptr(sout), ptr(flags), ptr(ninl))
    if max_trials is None:
        check(ctx.ptr, lib().cs_sim3_optimization(*args), "cs_sim3_optimization")
        res = [(sout[f].copy(), flags[off[f]:off[f + 1]].copy(), int(ninl[f])) for f in range(F)]
    else:
        trace, ntr, sys0 = np.zeros((F, max(max_trials, 1), 7)), np.zeros(F, np.int32), np.zeros((F, 36))
        check(ctx.ptr, lib().cs_sim3_optimization_trace(*args, max_trials, ptr(trace), ptr(ntr), ptr(sys0)), "cs_sim3_optimization_trace")
        res = [(sout[f].copy(), flags[off[f]:off[f + 1]].copy(), int(ninl[f]), trace[f, :min(int(ntr[f]), max_trials)].copy(), int(ntr[f]), sys0[f].copy()) for f in range(F)]
    return res[0] if single else res


MIN_FEAT = 100  # Optimizer.cc:2600


def build_essential_graph(flat):
    """The vertices and edges Optimizer::OptimizeEssentialGraph inserts (Optimizer.cc:2603-2776) from a flattened map:
    flat = {"kfs": [per key frame, in the order of pMap->GetAllKeyFrames(): {"mnId", "parent" (mnId or None), "loop_edges" (GetLoopEdges() in its iteration order),
    "covisibles" (GetCovisiblesByWeight(100) in its order), "children" (mnIds), "weights" ({mnId: GetWeight}, needed for the members of LoopConnections), "bad" (optional)}],
    "bad" (mnIds of bad key frames that are not in kfs but may appear among covisibles), "loop_connections" ([(mnId, [mnId, ...]), ...] in std::map / std::set iteration order),
    "loop_kf", "cur_kf" (mnIds), "Scw" ({mnId: 8 numbers}: CorrectedSim3 where the key frame has an entry, Sim3(Rcw, tcw, 1.0) otherwise), "non_corrected" ({mnId: 8 numbers})}.
    Vertex v is kfs[v].  Returns {"mnId" (n,), "edge_i", "edge_j" (m,) int32, "edge_kind" (m,) u8, "fixed_vertex", "Scw" (n,8), "Snc" (n,8), "has_nc" (n,) u8}.
    A bad key frame in kfs, or an edge to a key frame that is not in kfs, raises ValueError: the reference dereferences a null vertex there (:2791)."""
    kfs = flat["kfs"]
    index = {}
    for v, kf in enumerate(kfs):
        if kf.get("bad"):
            raise ValueError("build_essential_graph: key frame %d is bad; the reference gives it no vertex and dereferences a null pointer at Optimizer.cc:2791" % kf["mnId"])
        if kf["mnId"] in index:
            raise ValueError("build_essential_graph: key frame %d appears twice" % kf["mnId"])
        index[kf["mnId"]] = v
    bad = set(flat.get("bad", ()))
    loop_kf, cur_kf = flat["loop_kf"], flat["cur_kf"]

    def vertex(mnId):
        if mnId not in index:
            raise ValueError("build_essential_graph: key frame %d is %s; an edge to it has a null vertex in the reference" % (mnId, "bad" if mnId in bad else "not in the map"))
        return index[mnId]

    vertex(loop_kf), vertex(cur_kf)
    ei, ej, kind, inserted = [], [], [], set()
    for i, conns in flat["loop_connections"]:  # :2645-2673
        for j in conns:
            if (i != cur_kf or j != loop_kf) and kfs[vertex(i)]["weights"].get(j, 0) < MIN_FEAT:
                continue
            ei.append(vertex(i)), ej.append(vertex(j)), kind.append(0)
            inserted.add((min(i, j), max(i, j)))
    for kf in kfs:  # :2676-2776
        i, parent = kf["mnId"], kf["parent"]
        if parent is not None:
            ei.append(index[i]), ej.append(vertex(parent)), kind.append(1)
        for l in kf["loop_edges"]:
            if l < i:
                ei.append(index[i]), ej.append(vertex(l)), kind.append(1)
        for nb in kf["covisibles"]:
            if nb is not None and nb != parent and nb not in kf["children"] and nb not in kf["loop_edges"]:
                if nb not in bad and nb < i:
                    if (min(i, nb), max(i, nb)) in inserted:
                        continue
                    ei.append(index[i]), ej.append(vertex(nb)), kind.append(1)
    n = len(kfs)
    Scw = np.ascontiguousarray([np.asarray(flat["Scw"][kf["mnId"]], np.float64).reshape(8) for kf in kfs]).reshape(n, 8)
    Snc, has = np.zeros((n, 8)), np.zeros(n, np.uint8)
    for mnId, S in flat["non_corrected"].items():
        if mnId in index:
            Snc[index[mnId]] = np.asarray(S, np.float64).reshape(8)
            has[index[mnId]] = 1
    return {"mnId": np.array([kf["mnId"] for kf in kfs], np.int64), "edge_i": np.array(ei, np.int32), "edge_j": np.array(ej, np.int32), "edge_kind": np.array(kind, np.uint8),
            "fixed_vertex": index[loop_kf], "Scw": Scw, "Snc": Snc, "has_nc": has}


class _EgStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("trials", C.c_int), ("accepted", C.c_int), ("rejected", C.c_int), ("levels", C.c_int), ("l_blocks", C.c_int), ("h_blocks", C.c_int),
                ("launches_per_trial", C.c_int), ("chi2_first", C.c_double), ("chi2_last", C.c_double), ("lambda_last", C.c_double), ("trial_accepted", C.c_uint8 * 256)]


class EssentialGraph(Handle):
    """cs_essential_graph: the structure of one pose graph (a dict as build_essential_graph returns), analysed once; optimize() may run any number of times."""
    HANDLE, DESTROY = "_h", "cs_essential_graph_destroy"

    def __init__(self, graph, fix_scale, ctx=None, device=0):
        self.ctx = ctx or _lib.Context(device)
        self.n = len(graph["Scw"])
        ei, ej, kind = (np.ascontiguousarray(graph["edge_i"], np.int32), np.ascontiguousarray(graph["edge_j"], np.int32), np.ascontiguousarray(graph["edge_kind"], np.uint8))
        if not (len(ei) == len(ej) == len(kind)):
            raise ValueError("EssentialGraph: edge_i, edge_j and edge_kind differ in length")
        self.m = len(ei)
        self._h = C.c_void_p()
        check(self.ctx.ptr, lib().cs_essential_graph_create(self.ctx.ptr, self.n, len(ei), ptr(ei), ptr(ej), ptr(kind), int(graph["fixed_vertex"]),
                                                            int(bool(fix_scale)), C.byref(self._h)), "cs_essential_graph_create")

    def optimize(self, Scw, Snc, has_nc, iterations=20):
        """-> (sim3_out (n,8), Tiw (n,3,4) float32, stats)"""
        n = self.n
        Scw, Snc, has = np.ascontiguousarray(Scw, np.float64).reshape(-1, 8), np.ascontiguousarray(Snc, np.float64).reshape(-1, 8), np.ascontiguousarray(has_nc, np.uint8).reshape(-1)
        if not (len(Scw) == len(Snc) == len(has) == n):
            raise ValueError("EssentialGraph.optimize: Scw, Snc and has_nc need one row per vertex")
        out, Tiw, st = np.zeros((n, 8)), np.zeros((n, 3, 4), np.float32), _EgStats()
        check(self.ctx.ptr, lib().cs_essential_graph_optimize(self.ctx.ptr, self._h, ptr(Scw), ptr(Snc), ptr(has), int(iterations), ptr(out),
                                                              ptr(Tiw), C.byref(st)), "cs_essential_graph_optimize")
        stats = {k: getattr(st, k) for k, _ in _EgStats._fields_[:-1]}
        stats["sequence"] = [int(st.trial_accepted[k]) for k in range(min(st.trials, 256))]
        return out, Tiw, stats

    def solve(self, J, err, lam):
        """cs_essential_graph_solve (include/cubeslam_hip/essential_graph_solve.h), a test probe: one (H + lam I) x = b of the optimiser's trial from J (m, 14, 7) -- (m, 2, 7, 7)
        as eg_linearize lays it out -- and err (m, 7), through the optimiser's own assembly, factor and back-substitution launches -> (x (n, 7) by vertex, status)."""
        J, err = np.ascontiguousarray(J, np.float64).reshape(-1, 14, 7), np.ascontiguousarray(err, np.float64).reshape(-1, 7)
        if not (len(J) == len(err) == self.m):
            raise ValueError("EssentialGraph.solve: J and err need one row per edge")
        x, status = np.zeros((self.n, 7)), C.c_int(-1)
        check(self.ctx.ptr, lib().cs_essential_graph_solve(self.ctx.ptr, self._h, ptr(J), ptr(err), float(lam), ptr(x), C.byref(status)), "cs_essential_graph_solve")
        return x, status.value


def correct_points(P, ref_vertex, Scw, sim3_out, ctx=None, device=0):
    """Optimizer.cc:2824-2831 for every point: (float) sim3_out[r].inverse().map(Scw[r].map(P)); P (np,3) = toVector3d of the float positions, ref_vertex (np,) the vertex of nIDr."""
    ctx = ctx or _lib.Context(device)
    P, ref = np.ascontiguousarray(P, np.float64).reshape(-1, 3), np.ascontiguousarray(ref_vertex, np.int32).reshape(-1)
    Scw, out = np.ascontiguousarray(Scw, np.float64).reshape(-1, 8), np.ascontiguousarray(sim3_out, np.float64).reshape(-1, 8)
    if len(P) != len(ref) or Scw.shape != out.shape:
        raise ValueError("correct_points: one ref_vertex per point, one corrected Sim3 per Scw")
    res = np.zeros((len(P), 3), np.float32)
    check(ctx.ptr, lib().cs_sim3_correct_points(ctx.ptr, len(P), ptr(P), ptr(ref), len(Scw), ptr(Scw), ptr(out), ptr(res)),
          "cs_sim3_correct_points")
    return res


def sim3_log(S, ctx=None, device=0):
    """g2o::Sim3::log of (n,8) transforms -> (n,7) (omega, upsilon, sigma), on the device."""
    ctx = ctx or _lib.Context(device)
    S = np.ascontiguousarray(S, np.float64).reshape(-1, 8)
    out = np.zeros((len(S), 7))
    check(ctx.ptr, lib().cs_sim3_log(ctx.ptr, len(S), ptr(S), ptr(out)), "cs_sim3_log")
    return out


def sim3_exp(u, ctx=None, device=0):
    """g2o::Sim3(update) of (n,7) updates (omega, upsilon, sigma) -> (n,8) tx ty tz qx qy qz qw s, on the device (cs_sim3_exp, include/cubeslam_hip/sim3_opt_trace.h)."""
    ctx = ctx or _lib.Context(device)
    u = np.ascontiguousarray(u, np.float64).reshape(-1, 7)
    out = np.zeros((len(u), 8))
    check(ctx.ptr, lib().cs_sim3_exp(ctx.ptr, len(u), ptr(u), ptr(out)), "cs_sim3_exp")
    return out


def OptimizeEssentialGraph(flat, fix_scale, points=None, iterations=20, ctx=None, device=0):
    """Optimizer::OptimizeEssentialGraph (Optimizer.cc:2575-2836) on a flattened map (see build_essential_graph).  points: optional (P (np,3), nIDr (np,) mnIds), the
    float world positions and the reference key frame the caller chose per point (:2813-2822).
    Returns {"graph", "sim3" (n,8), "Tiw" (n,3,4) float32 -- what the caller hands to SetPose --, "points" (np,3) float32 or None -- for SetWorldPos --, "stats"}."""
    ctx = ctx or _lib.Context(device)
    g = build_essential_graph(flat)
    eg = EssentialGraph(g, fix_scale, ctx=ctx)
    try:
        sim3, Tiw, stats = eg.optimize(g["Scw"], g["Snc"], g["has_nc"], iterations)
    finally:
        eg.close()
    corrected = None
    if points is not None:
        index = {int(m): v for v, m in enumerate(g["mnId"])}
        try:
            ref = np.array([index[int(r)] for r in np.asarray(points[1]).reshape(-1)], np.int32)
        except KeyError as e:
            raise ValueError("OptimizeEssentialGraph: a point's reference key frame %s is not in the map" % e)
        corrected = correct_points(points[0], ref, g["Scw"], sim3, ctx=ctx)
    return {"graph": g, "sim3": sim3, "Tiw": Tiw, "points": corrected, "stats": stats}


def cuboid9_oplus(cub, upd, ctx=None, device=0):
    """g2o::VertexCuboid::oplusImpl for a batch (object_slam/include/object_slam/g2o_Object.h:193-204); cuboid = [t, q, half scale]."""
    ctx = ctx or _lib.Context(device)
    cub = np.ascontiguousarray(cub, np.float64).reshape(-1, 10); upd = np.ascontiguousarray(upd, np.float64).reshape(-1, 9)
    out = np.zeros_like(cub)
    check(ctx.ptr, lib().cs_cuboid9_oplus(ctx.ptr, len(cub), ptr(cub), ptr(upd), ptr(out)), "cs_cuboid9_oplus")
    return out


def cuboid9_edge_linearize(cam_Tcw, cub_global, cub_meas, jac=True, ctx=None, device=0):
    """g2o::EdgeSE3Cuboid::computeError (+ g2o's numeric Jacobians) for a batch of camera-object edges (g2o_Object.h:227-252)."""
    ctx = ctx or _lib.Context(device)
    T = np.ascontiguousarray(cam_Tcw, np.float64).reshape(-1, 7); g = np.ascontiguousarray(cub_global, np.float64).reshape(-1, 10)
    m = np.ascontiguousarray(cub_meas, np.float64).reshape(-1, 10)
    n = len(T)
    err = np.zeros((n, 9)); Jc = np.zeros((n, 9, 6)); Jq = np.zeros((n, 9, 9))
    check(ctx.ptr, lib().cs_cuboid9_edge_linearize(ctx.ptr, n, ptr(T), ptr(g), ptr(m), ptr(err),
                                                   ptr(Jc) if jac else None, ptr(Jq) if jac else None), "cs_cuboid9_edge_linearize")
    return (err, Jc, Jq) if jac else err
