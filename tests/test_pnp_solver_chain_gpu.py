"""GPU: Tracking::Relocalization (orb_object_slam/src/Tracking.cc:2876-3030) through the mirrors on three synthetic candidates -- SearchByBoW(pKF, F) -> PnPsolver
(evaluate_many: one call for the candidates that got a solver) -> PoseOptimization -> SearchByProjection(CurrentFrame, pKF, sFound, 10, 100) -- with nothing going back to host
arithmetic in between but the reference's own bookkeeping.  Candidate 0 shares fewer than 15 descriptors with the frame (:2913: no solver); candidate 1 shares descriptors but
not geometry (its RANSAC ends without consensus, bNoMore at :2949); candidate 2 sees the frame's points from a planted pose.  In one variant BoW pairs enough of them and
the optimised pose has nGood >= 50 at once (:3014); in the other BoW can pair only 40, nGood < 50, and the projection search of :2985-2991 finds the rest.  Only decisions are
asserted, no distances."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FX = FY = 500.0
CX, CY = 320.0, 240.0
BOUNDS = (0.0, 640.0, 0.0, 480.0)
SF = np.float32(1.2) ** np.arange(8, dtype=np.float32)
LOG_SF = float(np.float32(np.log(1.2)))


def _keys(uv):
    from cube_slam_amd.orb import KEYPOINT_DTYPE
    k = np.zeros(len(uv), KEYPOINT_DTYPE)
    k["x"], k["y"], k["size"], k["octave"] = uv[:, 0], uv[:, 1], 31.0, 0
    return k


def _project(X):
    return np.stack([FX * X[:, 0] / X[:, 2] + CX, FY * X[:, 1] / X[:, 2] + CY], 1).astype(np.float32)


def _key_frame(Xw, desc, node):
    """A key frame at the world's origin (Rcw = I, tcw = 0): one key point per map point."""
    d = np.linalg.norm(Xw, axis=1).astype(np.float32)
    return {"keys": _keys(_project(Xw)), "desc": desc, "node": node.astype(np.int32), "Xw": Xw.astype(np.float32), "max_d": (d * np.float32(1.05)).astype(np.float32),
            "min_d": (d * np.float32(1.05) / SF[-1]).astype(np.float32)}


def _scene(n_bow):
    """The frame F at a planted pose, and three candidate key frames; n_bow = how many features of the planted candidate lie in the vocabulary nodes of their twins in F."""
    rng = np.random.RandomState(23)
    n = 150
    z = rng.uniform(4.0, 8.0, n)
    Xw = np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], 1)
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    node = np.arange(n)
    flip = lambda d, k: d ^ (np.uint8(1) << rng.randint(0, 8, d.shape).astype(np.uint8)) * (rng.rand(*d.shape) < k / 32.0).astype(np.uint8)
    a = np.deg2rad(3.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]); t = np.array([0.12, -0.08, 0.15])
    uv = _project(Xw @ R.T + t) + rng.normal(size=(n, 2)).astype(np.float32) * np.float32(0.2)
    F = {"keys": _keys(uv), "desc": flip(desc, 3), "node": node.astype(np.int32)}
    node2 = node.copy(); node2[n_bow:] += 1000
    planted = _key_frame(Xw, desc, node2)
    d0 = rng.randint(0, 256, (n, 32)).astype(np.uint8); d0[:10] = flip(desc[:10], 2)
    few = _key_frame(Xw + rng.normal(size=Xw.shape) * 0.01, d0, node)
    zc = rng.uniform(4.0, 8.0, n)
    Xc = np.stack([rng.uniform(-0.4, 0.4, n) * zc, rng.uniform(-0.3, 0.3, n) * zc, zc], 1)
    d1 = rng.randint(0, 256, (n, 32)).astype(np.uint8); d1[:21] = flip(desc[:21], 2)
    no_geometry = _key_frame(Xc, d1, node)
    return F, [few, no_geometry, planted]


def _pose7(T):
    R = T[:3, :3].astype(np.float64)
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    return np.concatenate([T[:3, 3].astype(np.float64), [(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w]])


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("n_bow,rescued", [(140, False), (40, True)])
def test_relocalization_chain(ctx, n_bow, rescued):
    from cube_slam_amd.matcher import ORBmatcher
    from cube_slam_amd.optimizer import PoseOptimization
    from cube_slam_amd.pnp_solver import PnPsolver
    import cube_slam_amd.pnp_solver as M
    F, cands = _scene(n_bow)
    nF = len(F["keys"])
    matcher = ORBmatcher(0.75, True, ctx=ctx)
    mF = ORBmatcher(0.9, True, ctx=ctx); mF.set_frame(F["keys"], F["desc"], BOUNDS)
    K4 = (FX, FY, CX, CY)

    # :2905-2928: SearchByBoW per candidate, a solver where there are at least 15 matches
    discarded, reason, solvers, matches, rng = [], {}, {}, {}, np.random.RandomState(5)
    for i, c in enumerate(cands):
        mf, nmatches = matcher.SearchByBoW(c["keys"], c["desc"], c["node"], np.zeros(len(c["keys"]), np.uint8), F["keys"], F["desc"], F["node"])
        matches[i] = mf
        if nmatches < 15:
            discarded.append(True); reason[i] = "bow"
            continue
        discarded.append(False)
        idx = np.nonzero(mf >= 0)[0]  # the constructor's filter :79-101 (every map point is good)
        s = PnPsolver(c["Xw"][mf[idx]], np.stack([F["keys"]["x"][idx], F["keys"]["y"][idx]], 1), (SF * SF)[F["keys"]["octave"][idx]], K4, idx, nF, ctx=ctx)
        s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
        s.draw_quads(lambda lo, hi: int(rng.randint(lo, hi + 1)))
        solvers[i] = s
    assert reason == {0: "bow"} and sorted(solvers) == [1, 2] and solvers[1].N == 21
    assert (solvers[2].N >= 100) if not rescued else (15 <= solvers[2].N <= 40)
    calls, real = [], M.solver_evaluate
    M.solver_evaluate = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        PnPsolver.evaluate_many([solvers[i] for i in sorted(solvers)], ctx)  # after the SearchByBoW loop: one device call for the whole round-robin

        # :2937-3020
        n_cand, matched, n_good_first, n_additional, n_good = len(solvers), None, 0, 0, 0
        while n_cand > 0 and matched is None:
            for i, c in enumerate(cands):
                if discarded[i]:
                    continue
                Tcw, bNoMore, vbInliers, nInliers = solvers[i].iterate(5)
                if bNoMore:
                    discarded[i] = True; n_cand -= 1; reason[i] = "ransac"
                if Tcw is None:
                    continue
                mp = np.where(vbInliers, matches[i], -1)  # mCurrentFrame.mvpMapPoints
                def optimise(mp, pose):
                    j = np.nonzero(mp >= 0)[0]
                    obs = np.stack([F["keys"]["x"][j], F["keys"]["y"][j], np.full(len(j), -1.0)], 1)
                    pose, out, n = PoseOptimization([{"Xw": c["Xw"][mp[j]], "obs": obs, "inv_sigma2": np.ones(len(j)), "intr": K4 + (0.0,), "pose": pose}], ctx=ctx)[0]
                    return pose, j[out != 0], n
                pose, outliers, n_good = optimise(mp, _pose7(Tcw))
                n_good_first = n_good
                if n_good < 10:
                    continue
                mp[outliers] = -1
                if n_good < 50:  # :2982-2991
                    Rcw, tcw = _rot(pose[3:]), pose[:3]
                    skip = np.zeros(len(c["Xw"]), np.uint8); skip[mp[mp >= 0]] = 1  # sFound
                    tm, n_additional, _ = mF.SearchByProjectionReloc(Rcw.astype(np.float32), tcw.astype(np.float32), (-Rcw.T @ tcw).astype(np.float32), c["Xw"], c["min_d"], c["max_d"], skip,
                                                                     c["keys"]["angle"], c["desc"], FX, FY, CX, CY, LOG_SF, SF, 10.0, 100, (mp >= 0).astype(np.uint8))
                    if n_additional + n_good >= 50:
                        mp = np.where(mp >= 0, mp, tm)
                        pose, outliers, n_good = optimise(mp, pose)
                if n_good >= 50:
                    matched = i
                    break
    finally:
        M.solver_evaluate = real
    mF.close(); matcher.close()
    assert len(calls) == 1                              # evaluate_many made the one call; no iterate() evaluated anything again
    assert matched == 2 and n_good >= 50                # the planted candidate is accepted
    assert reason == {0: "bow", 1: "ransac"}           # the two others are discarded for the reference's reasons
    assert (n_good_first < 50 and n_additional + n_good_first >= 50) if rescued else (n_good_first >= 50 and n_additional == 0)
