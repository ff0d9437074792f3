"""Python host-side mirror of ORB_SLAM2::Sim3Solver (reference orb_object_slam/src/Sim3Solver.cc), the RANSAC of LoopClosing::ComputeSim3 (LoopClosing.cc:231-342), over
cs_sim3_solver_hypotheses: the hypotheses of all candidates of a loop are evaluated in one device call (evaluate_many), iterate() then walks a table of counts with the
reference's sequential rule (cs_sim3_solver_walk).  The constructor's filter (:60-101) stays the caller's: the solver is built over its results as flat arrays.  The triples the
reference draws from DUtils::Random are input: a table (set_triples), or draw_triples(random_int) over a caller's RandomInt(min, max).  ctx=None evaluates the same text
(csrc/horn_math.h) on the host, byte-equal to the device."""
import ctypes as C

import numpy as np

from ._lib import CubeSlamError, check, lib, ptr
from ._ransac import batch, cat, draw, f32, mask_bits, offsets, problem_slices


def max_iterations(probability, min_inliers, max_its, N):
    """mRansacMaxIts of SetRansacParameters (:118-133); 0 for N < min_inliers."""
    return lib().cs_sim3_solver_max_iterations(float(probability), int(min_inliers), int(max_its), int(N))


def solver_hypotheses(ctx, corr_off, X3Dc1, X3Dc2, max_err1, max_err2, K8, fix_scale, hyp_off, triples, n_inliers=None, sRt=None, mask=None):
    """cs_sim3_solver_hypotheses on flat arrays -> n_inliers[H], sRt[H, 13], inlier_mask (words; layout in include/cubeslam_hip.h).  ctx=None: the host evaluation."""
    co, ho, n, NC, H, words = batch(corr_off, hyp_off)
    x1, x2, e1, e2, k8 = f32(X3Dc1), f32(X3Dc2), f32(max_err1), f32(max_err2), f32(K8)
    fs = np.ascontiguousarray(fix_scale, np.uint8).reshape(-1); tr = np.ascontiguousarray(triples, np.int32).reshape(-1)
    if len(x1) != 3 * NC or len(x2) != 3 * NC or len(e1) != NC or len(e2) != NC or len(k8) != 8 * n or len(fs) != n or len(tr) != 3 * H:
        raise ValueError("array lengths do not fit corr_off / hyp_off")
    ni = np.zeros(max(H, 1), np.int32) if n_inliers is None else n_inliers
    st = np.zeros((max(H, 1), 13), np.float32) if sRt is None else sRt
    mk = np.zeros(max(words, 1), np.uint32) if mask is None else mask
    check(ctx.ptr if ctx is not None else None,
          lib().cs_sim3_solver_hypotheses(ctx.ptr if ctx is not None else None, n, ptr(co), ptr(x1), ptr(x2), ptr(e1), ptr(e2),
                                          ptr(k8), ptr(fs), ptr(ho), ptr(tr), ptr(ni), ptr(st), ptr(mk)),
          "cs_sim3_solver_hypotheses")
    return ni[:H], st[:H], mk[:words]


class Sim3Solver:
    """Members under the reference's names.  X3Dc1 / X3Dc2 (N, 3): mvX3Dc1 / mvX3Dc2; max_err1 / 2: mvnMaxError1 / 2 (:85-86; std::vector<size_t> in this reference: float(int(9.210 * sigma2))); K1 / K2: fx fy cx cy of mK1 / mK2;
    mvnIndices1[N]: the index in vpMatched12 of every kept correspondence; mN1 = vpMatched12.size()."""

    def __init__(self, X3Dc1, X3Dc2, max_err1, max_err2, K1, K2, mvnIndices1, mN1, bFixScale=False, ctx=None):
        self.ctx = ctx
        self.mvX3Dc1 = np.ascontiguousarray(X3Dc1, np.float32).reshape(-1, 3)
        self.mvX3Dc2 = np.ascontiguousarray(X3Dc2, np.float32).reshape(-1, 3)
        self.N = len(self.mvX3Dc1)
        self.mvnMaxError1 = np.ascontiguousarray(max_err1, np.float32).reshape(-1)
        self.mvnMaxError2 = np.ascontiguousarray(max_err2, np.float32).reshape(-1)
        self.K8 = np.concatenate([np.asarray(K1, np.float32).reshape(4), np.asarray(K2, np.float32).reshape(4)])
        self.mvnIndices1 = np.ascontiguousarray(mvnIndices1, np.int64).reshape(-1)
        self.mN1 = int(mN1)
        if not (len(self.mvX3Dc2) == len(self.mvnMaxError1) == len(self.mvnMaxError2) == len(self.mvnIndices1) == self.N):
            raise ValueError("one entry per correspondence in every array")
        if self.N and (self.mvnIndices1.min() < 0 or self.mvnIndices1.max() >= self.mN1):
            raise ValueError("mvnIndices1 outside 0..mN1 - 1")
        self.mbFixScale = bool(bFixScale)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self._best = -1
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.mRansacProb, self.mRansacMinInliers = probability, int(minInliers)
        self.mRansacMaxIts = max_iterations(probability, minInliers, maxIterations, self.N)
        self.mnIterations = 0
        self.triples = None
        self._table = None

    # ---- the triples
    def set_triples(self, triples):
        """The three indices of each of the mRansacMaxIts iterations, in drawing order."""
        t = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
        if len(t) != self.mRansacMaxIts:
            raise ValueError("%d triples for mRansacMaxIts = %d" % (len(t), self.mRansacMaxIts))
        self.triples, self._table = t, None

    def draw_triples(self, random_int):
        """:161-175 for every iteration: the partial Fisher-Yates over random_int(min, max), DUtils::Random::RandomInt."""
        t = draw(self.N, 3, self.mRansacMaxIts, random_int)
        self.set_triples(t)
        return t

    # ---- the table of all hypotheses
    @staticmethod
    def evaluate_many(solvers, ctx=None):
        """One cs_sim3_solver_hypotheses for the tables of all solvers (the candidates of one ComputeSim3).  ctx=None: the context of the first solver, the host when it has none."""
        solvers = list(solvers)
        if not solvers:
            return
        ctx = ctx if ctx is not None else solvers[0].ctx
        for s in solvers:
            if s.mRansacMaxIts and s.triples is None:
                raise CubeSlamError("Sim3Solver: no triples (set_triples or draw_triples)")
        ho = offsets(s.mRansacMaxIts for s in solvers)
        ni, sRt, mk = solver_hypotheses(ctx, offsets(s.N for s in solvers), cat([s.mvX3Dc1 for s in solvers], np.float32, 3), cat([s.mvX3Dc2 for s in solvers], np.float32, 3),
                                        cat([s.mvnMaxError1 for s in solvers], np.float32, 1), cat([s.mvnMaxError2 for s in solvers], np.float32, 1),
                                        cat([s.K8 for s in solvers], np.float32, 8), [s.mbFixScale for s in solvers], ho,
                                        cat([s.triples for s in solvers if s.mRansacMaxIts], np.int32, 3))
        for s, t in zip(solvers, problem_slices({"n": ni, "sRt": sRt, "mask": mk}, ho, [s.N for s in solvers], masks=("mask",))):
            s._table = (t["n"], t["sRt"], t["mask"])

    def table(self):
        if self._table is None:
            Sim3Solver.evaluate_many([self])
        return self._table

    # ---- the reference's interface
    def iterate(self, nIterations):
        """-> (mBestT12 (4, 4) or None, bNoMore, vbInliers[mN1], nInliers)."""
        vbInliers = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers:  # :144
            return None, True, vbInliers, 0
        counts, _, masks = self.table()
        it, best, h, nomore = C.c_int(self.mnIterations), C.c_int(self.mnBestInliers), C.c_int(self._best), C.c_int(0)
        t = lib().cs_sim3_solver_walk(ptr(counts), self.mRansacMaxIts, self.mRansacMinInliers, C.byref(it), C.byref(best), C.byref(h), int(nIterations), C.byref(nomore))
        self.mnIterations, self.mnBestInliers, self._best = it.value, best.value, h.value
        if t < 0:
            return None, bool(nomore.value), vbInliers, 0
        vbInliers[self.mvnIndices1[mask_bits(masks[t], self.N)]] = True
        return self._T12(t), False, vbInliers, int(counts[t])

    def find(self):
        """-> (mBestT12 or None, vbInliers12, nInliers)."""
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n

    def _T12(self, t):
        sRt = self.table()[1][t]
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = (sRt[1:10].astype(np.float64) * np.float64(sRt[0])).astype(np.float32).reshape(3, 3)  # sR = ms12i * mR12i
        T[:3, 3] = sRt[10:13]
        return T

    def _best_sRt(self):
        if self._best < 0:
            raise CubeSlamError("Sim3Solver: no best hypothesis yet")
        return self.table()[1][self._best]

    def GetEstimatedRotation(self):
        return self._best_sRt()[1:10].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self._best_sRt()[10:13].copy()

    def GetEstimatedScale(self):
        return np.float32(self._best_sRt()[0])

    def best_inliers(self):
        """mvbBestInliers[N]."""
        return mask_bits(self.table()[2][self._best], self.N)
