"""GPU: LoopClosing::ComputeSim3 (orb_object_slam/src/LoopClosing.cc:231-342) through the mirrors on three synthetic loop candidates -- SearchByBoW(pKF1, pKF2) -> Sim3Solver
(evaluate_many: one call for the candidates that got a solver) -> SearchBySim3 -> OptimizeSim3 -- with nothing going back to host arithmetic in between but the reference's own
bookkeeping.  Candidate 0 shares too few descriptors with the current key frame (nmatches < 20, :266: it gets no solver); candidate 1 shares descriptors but not geometry (21
matches whose map points lie anywhere: its RANSAC ends without consensus, bNoMore at :300); candidate 2 sees the current key frame's points through a planted similarity and is
the one accepted, with at least 20 inliers after the optimisation (:322).  Only decisions are asserted, no distances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FX = FY = 500.0
CX, CY = 320.0, 240.0
BOUNDS = (0.0, 640.0, 0.0, 480.0)
SF = np.float32(1.2) ** np.arange(8, dtype=np.float32)
LOG_SF = float(np.float32(np.log(1.2)))
SIGMA2 = SF * SF


def _keys(uv):
    from cube_slam_amd.orb import KEYPOINT_DTYPE
    k = np.zeros(len(uv), KEYPOINT_DTYPE)
    k["x"], k["y"], k["size"], k["octave"] = uv[:, 0], uv[:, 1], 31.0, 0
    return k


def _project(X):
    return np.stack([FX * X[:, 0] / X[:, 2] + CX, FY * X[:, 1] / X[:, 2] + CY], 1).astype(np.float32)


def _frame(X, desc, node):
    """A key frame at the origin of its own map (Rcw = I, tcw = 0): its map points are its camera-frame points X; one key point per map point."""
    d = np.linalg.norm(X, axis=1).astype(np.float32)
    return {"keys": _keys(_project(X)), "desc": desc, "node": node.astype(np.int32), "X": X.astype(np.float32), "max_d": (d * np.float32(1.05)).astype(np.float32),
            "min_d": (d * np.float32(1.05) / SF[-1]).astype(np.float32)}


def _scene():
    rng = np.random.RandomState(17)
    n = 150
    z = rng.uniform(4.0, 8.0, n)
    X1 = np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], 1)
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    node = np.arange(n)
    flip = lambda d, k: d ^ (np.uint8(1) << rng.randint(0, 8, d.shape).astype(np.uint8)) * (rng.rand(*d.shape) < k / 32.0).astype(np.uint8)
    cur = _frame(X1, desc, node)
    # candidate 2: X1 = s R X2 + t.  30 of its features sit in other vocabulary nodes than their twins: SearchByBoW cannot pair them, SearchBySim3 can
    a = np.deg2rad(4.0); s = 0.95
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]); t = np.array([0.15, -0.1, 0.2])
    X2 = (X1 - t) @ R / s
    node2 = node.copy(); node2[120:] += 1000
    planted = _frame(X2, flip(desc, 3), node2)
    # candidate 0: 10 shared descriptors, the others its own
    d0 = rng.randint(0, 256, (n, 32)).astype(np.uint8); d0[:10] = flip(desc[:10], 2)
    few = _frame(X1 + rng.normal(size=X1.shape) * 0.01, d0, node)
    # candidate 1: 21 shared descriptors, map points anywhere in its frustum
    zc = rng.uniform(4.0, 8.0, n)
    Xc = np.stack([rng.uniform(-0.4, 0.4, n) * zc, rng.uniform(-0.3, 0.3, n) * zc, zc], 1)
    d1 = rng.randint(0, 256, (n, 32)).astype(np.uint8); d1[:21] = flip(desc[:21], 2)
    no_consensus = _frame(Xc, d1, node)
    return cur, [few, no_consensus, planted]


def _quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def test_compute_sim3_chain(ctx):
    from cube_slam_amd.matcher import ORBmatcher
    from cube_slam_amd.optimizer import OptimizeSim3
    from cube_slam_amd.sim3_solver import Sim3Solver
    cur, cands = _scene()
    n1 = len(cur["keys"])
    matcher = ORBmatcher(0.75, True, ctx=ctx)
    m1 = ORBmatcher(0.75, True, ctx=ctx); m1.set_frame(cur["keys"], cur["desc"], BOUNDS)
    no_skip = np.zeros(n1, np.uint8)
    K4 = (FX, FY, CX, CY)
    eye, zero = np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)

    # :247-279: SearchByBoW per candidate, a solver where there are at least 20 matches
    discarded, reason, solvers, matches, rng = [], {}, {}, {}, np.random.RandomState(3)
    for i, c in enumerate(cands):
        m12, nmatches = matcher.SearchByBoWKeyFrames(cur["keys"], cur["desc"], cur["node"], no_skip, c["keys"], c["desc"], c["node"], np.zeros(len(c["keys"]), np.uint8))
        matches[i] = m12
        if nmatches < 20:
            discarded.append(True); reason[i] = "bow"
            continue
        discarded.append(False)
        idx1 = np.nonzero(m12 >= 0)[0]  # the constructor's filter :60-101 (every map point is good and has its key point)
        thr = lambda k: np.floor(9.210 * SIGMA2[k["octave"]].astype(np.float64)).astype(np.float32)  # std::vector<size_t> mvnMaxError
        s = Sim3Solver(cur["X"][idx1], c["X"][m12[idx1]], thr(cur["keys"][idx1]), thr(c["keys"][m12[idx1]]), K4, K4, idx1, n1, bFixScale=False, ctx=ctx)
        s.SetRansacParameters(0.99, 20, 300)
        s.draw_triples(lambda lo, hi: int(rng.randint(lo, hi + 1)))
        solvers[i] = s
    assert reason == {0: "bow"} and sorted(solvers) == [1, 2] and solvers[1].N == 21 and solvers[2].N >= 100
    Sim3Solver.evaluate_many([solvers[i] for i in sorted(solvers)], ctx)  # after the SearchByBoW loop: one device call for the whole round-robin

    # :283-342
    n_cand, matched, n_opt, n_new = len(solvers), None, 0, 0
    while n_cand > 0 and matched is None:
        for i, c in enumerate(cands):
            if discarded[i]:
                continue
            Scm, bNoMore, vbInliers, nInliers = solvers[i].iterate(5)
            if bNoMore:
                discarded[i] = True; n_cand -= 1; reason[i] = "ransac"
            if Scm is None:
                continue
            vp = np.where(vbInliers, matches[i], -1)
            Rm, t, sc = solvers[i].GetEstimatedRotation(), solvers[i].GetEstimatedTranslation(), solvers[i].GetEstimatedScale()
            m2 = ORBmatcher(0.75, True, ctx=ctx); m2.set_frame(c["keys"], c["desc"], BOUNDS)
            sR12 = (Rm.astype(np.float64) * float(sc)).astype(np.float32)
            sR21 = (Rm.T.astype(np.float64) * (1.0 / float(sc))).astype(np.float32)
            t21 = (-(sR21.astype(np.float64) @ t.astype(np.float64))).astype(np.float32)
            skip1 = (vp >= 0).astype(np.uint8)
            skip2 = np.zeros(len(c["keys"]), np.uint8); skip2[vp[vp >= 0]] = 1
            new12, n_found, _ = m1.SearchBySim3(m2, eye, zero, eye, zero, sR12, t, sR21, t21, (cur["X"], cur["min_d"], cur["max_d"], skip1, cur["desc"]),
                                                (c["X"], c["min_d"], c["max_d"], skip2, c["desc"]), FX, FY, CX, CY, LOG_SF, SF, 7.5)
            m2.close()
            n_new = int(((new12 >= 0) & (vp < 0)).sum())
            vp = np.where(vp >= 0, vp, new12)
            i1 = np.nonzero(vp >= 0)[0]
            res = OptimizeSim3({"P1c": cur["X"][i1], "P2c": c["X"][vp[i1]], "obs1": np.stack([cur["keys"]["x"][i1], cur["keys"]["y"][i1]], 1),
                                "obs2": np.stack([c["keys"]["x"][vp[i1]], c["keys"]["y"][vp[i1]]], 1), "inv_sigma2_1": np.ones(len(i1)), "inv_sigma2_2": np.ones(len(i1)),
                                "intrinsics": K4 + K4, "sim3_in": np.concatenate([t.astype(np.float64), _quat(Rm.astype(np.float64)), [float(sc)]]), "th2": 10.0, "fix_scale": False},
                               ctx=ctx)
            n_opt = res[2]
            if n_opt >= 20:
                matched = i
                break
    m1.close(); matcher.close()
    assert matched == 2 and n_opt >= 20                 # the planted candidate is accepted
    assert reason == {0: "bow", 1: "ransac"}           # the two others are discarded for the reference's reasons
    assert n_new >= 1                                   # SearchBySim3 added pairs SearchByBoW could not make
