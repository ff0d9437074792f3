"""Python host-side mirror of ORB_SLAM2::PnPsolver (reference orb_object_slam/src/PnPsolver.cc), the RANSAC over EPnP of Tracking::Relocalization (Tracking.cc:2876-3030), over
cs_pnp_solver_evaluate: the hypotheses of all candidates of a relocalisation, and every distinct Refine(), are evaluated in one device call (evaluate_many); iterate() then walks
the two tables of counts with the reference's sequential rule (cs_pnp_solver_walk).  The constructor's filter (:79-101) stays the caller's: the solver is built over its results as
flat arrays.  The quads the reference draws from DUtils::Random are input: a table (set_quads), or draw_quads(random_int) over a caller's RandomInt(min, max).  ctx=None evaluates
the same text (csrc/epnp_math.h, csrc/cv_svd_math.h) on the host, byte-equal to the device."""
import ctypes as C

import numpy as np

from ._lib import CubeSlamError, check, lib, ptr
from ._ransac import batch, cat, draw, f32, i32, mask_bits, offsets, problem_slices

STATUS_QR_SINGULAR, STATUS_REFINE_QR_SINGULAR, STATUS_RECORD = 1, 2, 4


def ransac_parameters(probability, minInliers, maxIterations, minSet, epsilon, N):
    """SetRansacParameters (:120-151) -> (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon)."""
    mi, its, eps = C.c_int(), C.c_int(), C.c_float()
    check(None, lib().cs_pnp_solver_ransac_parameters(float(probability), int(minInliers), int(maxIterations), int(minSet), float(epsilon), int(N), C.byref(mi), C.byref(its), C.byref(eps)), "cs_pnp_solver_ransac_parameters")
    return mi.value, its.value, np.float32(eps.value)


def walk(n_inliers, refined_n, ransac_max_its, min_inliers, mnIterations, mnBestInliers, best_hypothesis, nIterations):
    """cs_pnp_solver_walk -> (hypothesis | -1 | -2, refined, bNoMore, mnIterations, mnBestInliers, best_hypothesis)."""
    ni = np.ascontiguousarray(n_inliers, np.int32); rn = np.ascontiguousarray(refined_n, np.int32)
    it, best, h, nomore, ref = C.c_int(mnIterations), C.c_int(mnBestInliers), C.c_int(best_hypothesis), C.c_int(0), C.c_int(0)
    t = lib().cs_pnp_solver_walk(ptr(ni), ptr(rn), len(ni), int(ransac_max_its), int(min_inliers), C.byref(it), C.byref(best), C.byref(h), int(nIterations),
                                 C.byref(nomore), C.byref(ref))
    return t, bool(ref.value), bool(nomore.value), it.value, best.value, h.value


def solver_evaluate(ctx, corr_off, P3Dw, P2D, max_err, K4, min_inliers, best_in, hyp_off, quads):
    """cs_pnp_solver_evaluate on flat arrays -> dict of n_inliers[H], Rt[H, 12], status[H], mask (words), refined_n[H], refined_Rt[H, 12], refined_mask (words; layout in
    include/cubeslam_hip.h).  ctx=None: the host evaluation."""
    co, ho, n, NC, H, words = batch(corr_off, hyp_off)
    x, u, e, k4, mi, bi, q = f32(P3Dw), f32(P2D), f32(max_err), f32(K4), i32(min_inliers), i32(best_in), i32(quads)
    if len(x) != 3 * NC or len(u) != 2 * NC or len(e) != NC or len(k4) != 4 * n or len(mi) != n or len(bi) != n or len(q) != 4 * H:
        raise ValueError("array lengths do not fit corr_off / hyp_off")
    out = {"n_inliers": np.zeros(max(H, 1), np.int32), "Rt": np.zeros((max(H, 1), 12), np.float64), "status": np.zeros(max(H, 1), np.uint32),
           "mask": np.zeros(max(words, 1), np.uint32), "refined_n": np.zeros(max(H, 1), np.int32), "refined_Rt": np.zeros((max(H, 1), 12), np.float64),
           "refined_mask": np.zeros(max(words, 1), np.uint32)}
    cp = ctx.ptr if ctx is not None else None
    check(cp, lib().cs_pnp_solver_evaluate(cp, n, ptr(co), ptr(x), ptr(u), ptr(e), ptr(k4), ptr(mi), ptr(bi),
                                           ptr(ho), ptr(q), ptr(out["n_inliers"]), ptr(out["Rt"]), ptr(out["status"]),
                                           ptr(out["mask"]), ptr(out["refined_n"]), ptr(out["refined_Rt"]), ptr(out["refined_mask"])),
          "cs_pnp_solver_evaluate")
    for k in ("n_inliers", "Rt", "status", "refined_n", "refined_Rt"):
        out[k] = out[k][:H]
    out["mask"], out["refined_mask"] = out["mask"][:words], out["refined_mask"][:words]
    return out


def _Tcw(Rt):
    """:216-222 / :292-298: the doubles of mRi, mti converted to CV_32F into a 4 x 4 identity."""
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = Rt[:9].astype(np.float32).reshape(3, 3)
    T[:3, 3] = Rt[9:12].astype(np.float32)
    return T


class PnPsolver:
    """Members under the reference's names.  P3Dw (N, 3): mvP3Dw; P2D (N, 2): mvP2D; sigma2[N]: mvSigma2; K = fu fv uc vc; mvKeyPointIndices[N]: the index in vpMapPointMatches of
    every kept correspondence; n_matches = mvpMapPointMatches.size().  random_int (optional): RandomInt(min, max), kept for quads drawn past the table."""

    def __init__(self, P3Dw, P2D, sigma2, K, mvKeyPointIndices, n_matches, ctx=None, random_int=None):
        self.ctx = ctx
        self.mvP3Dw = np.ascontiguousarray(P3Dw, np.float32).reshape(-1, 3)
        self.mvP2D = np.ascontiguousarray(P2D, np.float32).reshape(-1, 2)
        self.mvSigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1)
        self.N = len(self.mvP3Dw)
        self.K4 = np.asarray(K, np.float32).reshape(4)
        self.mvKeyPointIndices = np.ascontiguousarray(mvKeyPointIndices, np.int64).reshape(-1)
        self.n_matches = int(n_matches)
        if not (len(self.mvP2D) == len(self.mvSigma2) == len(self.mvKeyPointIndices) == self.N):
            raise ValueError("one entry per correspondence in every array")
        if self.N and (self.mvKeyPointIndices.min() < 0 or self.mvKeyPointIndices.max() >= self.n_matches):
            raise ValueError("mvKeyPointIndices outside 0..n_matches - 1")
        self.random_int = random_int
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        if minSet != 4:
            raise CubeSlamError("PnPsolver: EPnP hypotheses are drawn from 4 correspondences (minSet == 4)")
        self.mRansacProb, self.mRansacMinSet = probability, 4
        self.mRansacMinInliers, self.mRansacMaxIts, self.mRansacEpsilon = ransac_parameters(probability, minInliers, maxIterations, minSet, epsilon, self.N)
        self.mvMaxError = self.mvSigma2 * np.float32(th2)  # :155, float * float
        self.mnIterations, self.mnBestInliers, self._best = 0, 0, -1
        self.quads = np.zeros((0, 4), np.int32)
        self._table = None

    # ---- the quads
    def set_quads(self, quads):
        """The four indices of each iteration, in drawing order: at least mRansacMaxIts of them (iterate() calls made after a rejected success read further ones, :181)."""
        q = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
        if self.N >= self.mRansacMinInliers and len(q) < self.mRansacMaxIts:
            raise ValueError("%d quads for mRansacMaxIts = %d" % (len(q), self.mRansacMaxIts))
        self.quads, self._table = q, None

    def draw_quads(self, random_int, extra=5):
        """mRansacMaxIts + extra quads from random_int, which is kept for those a later iterate() needs."""
        self.random_int = random_int
        n = self.mRansacMaxIts + int(extra) if self.N >= max(self.mRansacMinInliers, 4) else 0
        self.set_quads(draw(self.N, 4, n, random_int))  # :187-200
        return self.quads

    # ---- the tables of all hypotheses
    @staticmethod
    def evaluate_many(solvers, ctx=None):
        """One cs_pnp_solver_evaluate for the hypotheses not yet evaluated of all solvers (the candidates of one Relocalization).  ctx=None: the context of the first solver,
        the host when it has none."""
        solvers = list(solvers)
        if not solvers:
            return
        ctx = ctx if ctx is not None else solvers[0].ctx
        done = [0 if s._table is None else len(s._table["n_inliers"]) for s in solvers]
        todo = [s.quads[d:] if s.N >= max(s.mRansacMinInliers, 4) else s.quads[:0] for s, d in zip(solvers, done)]
        if not any(len(t) for t in todo):
            return
        ho = offsets(len(t) for t in todo)
        best_in = [0 if s._table is None else int(max([0] + [c for c in s._table["n_inliers"] if c >= s.mRansacMinInliers])) for s in solvers]
        out = solver_evaluate(ctx, offsets(s.N for s in solvers), cat([s.mvP3Dw for s in solvers], np.float32, 3), cat([s.mvP2D for s in solvers], np.float32, 2),
                              cat([s.mvMaxError for s in solvers], np.float32, 1), cat([s.K4 for s in solvers], np.float32, 4), [s.mRansacMinInliers for s in solvers], best_in, ho,
                              cat(todo, np.int32, 4))
        for s, new in zip(solvers, problem_slices(out, ho, [s.N for s in solvers], masks=("mask", "refined_mask"))):
            s._table = new if s._table is None else {k: np.concatenate([s._table[k], new[k]]) for k in new}

    def table(self):
        if self._table is None or len(self._table["n_inliers"]) < len(self.quads):
            PnPsolver.evaluate_many([self])
        return self._table

    # ---- the reference's interface
    def iterate(self, nIterations):
        """-> (Tcw (4, 4) float32 or None, bNoMore, vbInliers[n_matches], nInliers)."""
        vbInliers = np.zeros(self.n_matches, bool)
        if self.N < self.mRansacMinInliers:  # :172
            return None, True, vbInliers, 0
        if not len(self.quads):
            raise CubeSlamError("PnPsolver: no quads (set_quads or draw_quads)")
        left = int(nIterations)
        while True:
            T = self.table()
            before = self.mnIterations
            t, refined, nomore, self.mnIterations, self.mnBestInliers, self._best = walk(T["n_inliers"], T["refined_n"], self.mRansacMaxIts, self.mRansacMinInliers, self.mnIterations,
                                                                                         self.mnBestInliers, self._best, left)
            if t != -2:
                break
            if self.random_int is None:
                raise CubeSlamError("PnPsolver: iterate() reads hypothesis %d and the table has %d quads (:181 runs past mRansacMaxIts after a success)" % (self.mnIterations, len(self.quads)))
            left -= self.mnIterations - before
            self.quads = np.concatenate([self.quads, draw(self.N, 4, 5, self.random_int)])
        if t < 0:
            return None, nomore, vbInliers, 0
        mask, Rt, n = (T["refined_mask"][t], T["refined_Rt"][t], T["refined_n"][t]) if refined else (T["mask"][t], T["Rt"][t], T["n_inliers"][t])
        vbInliers[self.mvKeyPointIndices[mask_bits(mask, self.N)]] = True
        return _Tcw(Rt), nomore, vbInliers, int(n)

    def find(self):
        """-> (Tcw or None, vbInliers, nInliers)."""
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n
