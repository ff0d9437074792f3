"""Python host-side mirror of ORB_SLAM2::Initializer (reference orb_object_slam/src/Initializer.cc), the two-view initialisation of Tracking::MonocularInitialization
(Tracking.cc:948-983), over cs_initializer_evaluate: the 2 x mMaxIterations hypotheses of every frame pair, the choice between homography and fundamental matrix and the CheckRT
passes of the chosen model's candidates are evaluated in one device call (evaluate_many); the decisions of ReconstructF / ReconstructH over the candidates' counts are then the
host's (cs_initializer_walk).  The sets of eight the reference draws from DUtils::Random are input: a table (set_sets), or draw_sets(random_int) over a caller's
RandomInt(min, max).  ctx=None evaluates the same text (csrc/initializer_math.h) on the host, byte-equal to the device."""
import ctypes as C

import numpy as np

from ._lib import CubeSlamError, check, lib, ptr
from ._ransac import batch, cat, draw, f32, i32, mask_bits, offsets

MODEL_NONE, MODEL_H, MODEL_F = -1, 0, 1
MAX_CAND = 8


def walk(model, n_cand, nGood, cos_parallax, N, minParallax=1.0, minTriangulated=50):
    """cs_initializer_walk -> (candidate | -1, parallax)."""
    g, c = np.ascontiguousarray(nGood, np.int32), np.ascontiguousarray(cos_parallax, np.float32)
    if len(g) < MAX_CAND or len(c) < MAX_CAND:
        raise ValueError("nGood and cos_parallax hold %d entries" % MAX_CAND)
    par = C.c_float()
    return lib().cs_initializer_walk(int(model), int(n_cand), ptr(g), ptr(c), int(N), float(minParallax), int(minTriangulated), C.byref(par)), np.float32(par.value)


def initializer_evaluate(ctx, key1_off, keys1, key2_off, keys2, corr_off, matches12, K9, sigma, hyp_off, sets):
    """cs_initializer_evaluate on flat arrays -> dict (layout in include/cubeslam_hip.h): score[2, H], matrix[2, H, 9], mask[2, words]; per problem model, best[P, 2], S[P, 2], RH,
    n_inliers, n_cand, cand_Rt[P, 8, 12], nGood[P, 8], cos_parallax[P, 8]; good_mask (words) and points (floats) per candidate.  ctx=None: the host evaluation."""
    co, ho, n, NC, H, words = batch(corr_off, hyp_off)
    k1o, k2o = i32(key1_off), i32(key2_off)
    if len(k1o) != n + 1 or len(k2o) != n + 1:
        raise ValueError("key1_off and key2_off must have one entry per problem and one more")
    a1, a2, mt, k9, sg, st = f32(keys1), f32(keys2), i32(matches12), f32(K9), f32(sigma), i32(sets)
    NK1, NK2 = (int(k1o[-1]), int(k2o[-1])) if n else (0, 0)
    if len(a1) != 2 * NK1 or len(a2) != 2 * NK2 or len(mt) != 2 * NC or len(k9) != 9 * n or len(sg) != n or len(st) != 8 * H:
        raise ValueError("array lengths do not fit the offsets")
    N = np.diff(co.astype(np.int64)) if n else np.zeros(0, np.int64)
    cwords = 0 if (N < 0).any() else int(MAX_CAND * ((N + 31) // 32).sum())
    out = {"score": np.zeros(max(2 * H, 1), np.float32), "matrix": np.zeros(max(18 * H, 1), np.float32), "mask": np.zeros(max(2 * words, 1), np.uint32),
           "model": np.zeros(max(n, 1), np.int32), "best": np.zeros(max(2 * n, 1), np.int32), "S": np.zeros(max(2 * n, 1), np.float32), "RH": np.zeros(max(n, 1), np.float32),
           "n_inliers": np.zeros(max(n, 1), np.int32), "n_cand": np.zeros(max(n, 1), np.int32), "cand_Rt": np.zeros(max(96 * n, 1), np.float32),
           "nGood": np.zeros(max(8 * n, 1), np.int32), "cos_parallax": np.zeros(max(8 * n, 1), np.float32), "good_mask": np.zeros(max(cwords, 1), np.uint32),
           "points": np.zeros(max(24 * max(NC, 0), 1), np.float32)}
    cp = ctx.ptr if ctx is not None else None
    o = out
    check(cp, lib().cs_initializer_evaluate(cp, n, ptr(k1o), ptr(a1), ptr(k2o), ptr(a2), ptr(co), ptr(mt), ptr(k9),
                                            ptr(sg), ptr(ho), ptr(st), ptr(o["score"]), ptr(o["matrix"]), ptr(o["mask"]),
                                            ptr(o["model"]), ptr(o["best"]), ptr(o["S"]), ptr(o["RH"]), ptr(o["n_inliers"]),
                                            ptr(o["n_cand"]), ptr(o["cand_Rt"]), ptr(o["nGood"]), ptr(o["cos_parallax"]),
                                            ptr(o["good_mask"]), ptr(o["points"])), "cs_initializer_evaluate")
    out["score"] = out["score"][:2 * H].reshape(2, H)
    out["matrix"] = out["matrix"][:18 * H].reshape(2, H, 9)
    out["mask"] = out["mask"][:2 * words].reshape(2, words)
    for k in ("model", "RH", "n_inliers", "n_cand"):
        out[k] = out[k][:n]
    out["best"], out["S"] = out["best"][:2 * n].reshape(n, 2), out["S"][:2 * n].reshape(n, 2)
    out["cand_Rt"] = out["cand_Rt"][:96 * n].reshape(n, 8, 12)
    out["nGood"], out["cos_parallax"] = out["nGood"][:8 * n].reshape(n, 8), out["cos_parallax"][:8 * n].reshape(n, 8)
    out["good_mask"], out["points"] = out["good_mask"][:cwords], out["points"][:24 * NC]
    return out


def problem_tables(out, co, ho):
    """The arrays of one call cut per problem: p -> dict with its hypotheses' score[2, nh], matrix[2, nh, 9], mask[2, nh, W], its per-problem values, good_mask[8, W] and
    points[8, N, 3] (copies)."""
    w0 = cw0 = 0
    for p in range(len(co) - 1):
        N, nh = int(co[p + 1] - co[p]), int(ho[p + 1] - ho[p])
        W = (N + 31) // 32
        t = {"score": out["score"][:, ho[p]:ho[p + 1]].copy(), "matrix": out["matrix"][:, ho[p]:ho[p + 1]].copy(), "mask": out["mask"][:, w0:w0 + nh * W].reshape(2, nh, W).copy(),
             "good_mask": out["good_mask"][cw0:cw0 + MAX_CAND * W].reshape(MAX_CAND, W).copy(),
             "points": out["points"][24 * int(co[p]):24 * int(co[p + 1])].reshape(MAX_CAND, N, 3).copy(), "N": N}
        for k in ("model", "best", "S", "RH", "n_inliers", "n_cand", "cand_Rt", "nGood", "cos_parallax"):
            t[k] = out[k][p].copy()
        w0 += nh * W; cw0 += MAX_CAND * W
        yield t


class Initializer:
    """Members under the reference's names.  ReferenceFrame_keys (n1, 2): the x, y of ReferenceFrame.mvKeysUn; K (3, 3); sigma, iterations as the constructor (:34-43).
    random_int (optional): RandomInt(min, max), from which Initialize draws its sets where no table was given."""

    def __init__(self, ReferenceFrame_keys, K, sigma=1.0, iterations=200, ctx=None, random_int=None):
        self.ctx = ctx
        self.mvKeys1 = np.ascontiguousarray(ReferenceFrame_keys, np.float32).reshape(-1, 2)
        self.mK = np.ascontiguousarray(K, np.float32).reshape(3, 3)
        self.mSigma = np.float32(sigma)
        self.mMaxIterations = int(iterations)
        self.random_int = random_int
        self.mvSets = None
        self._pending = self._table = None

    # ---- the sets
    def set_sets(self, sets):
        """The eight indices of each iteration (mvSets), in drawing order, for the next Initialize."""
        self.mvSets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)

    def draw_sets(self, random_int, N):
        """mMaxIterations sets over N correspondences from random_int (:83-98).  The reference seeds DUtils::Random once per process (SeedRandOnce(0)) and every later
        Initialize continues the stream: the caller's random_int carries that state."""
        self.set_sets(draw(int(N), 8, self.mMaxIterations, random_int))
        return self.mvSets

    # ---- one call for many frame pairs
    def prepare(self, CurrentFrame_keys, vMatches12):
        """:50-66: mvKeys2 and mvMatches12 of the next evaluation.  vMatches12[i] = the index in the current frame matched to key point i of the reference frame, or < 0."""
        self.mvKeys2 = np.ascontiguousarray(CurrentFrame_keys, np.float32).reshape(-1, 2)
        v = np.ascontiguousarray(vMatches12, np.int64).reshape(-1)
        if len(v) > len(self.mvKeys1):
            raise ValueError("vMatches12 is longer than the reference frame's key points")
        first = np.nonzero(v >= 0)[0]
        self.mvMatches12 = np.stack([first, v[first]], 1).astype(np.int32)
        N = len(self.mvMatches12)
        if N >= 8 and self.mvSets is None and self.random_int is not None:
            self.draw_sets(self.random_int, N)
        if N >= 8 and self.mvSets is None:
            raise CubeSlamError("Initializer: no sets (set_sets, draw_sets or random_int)")
        self._pending, self._table = (self.mvSets if N >= 8 else np.zeros((0, 8), np.int32)), None
        self.mvSets = None  # (a table serves one Initialize: the reference draws anew every time)

    @staticmethod
    def evaluate_many(initializers, ctx=None):
        """One cs_initializer_evaluate for all prepared initializers (the frame pairs tried at once).  ctx=None: the context of the first, the host when it has none."""
        its = [i for i in initializers if i._pending is not None]
        if not its:
            return
        ctx = ctx if ctx is not None else its[0].ctx
        co, ho = offsets(len(i.mvMatches12) for i in its), offsets(len(i._pending) for i in its)
        out = initializer_evaluate(ctx, offsets(len(i.mvKeys1) for i in its), cat([i.mvKeys1 for i in its], np.float32, 2), offsets(len(i.mvKeys2) for i in its),
                                   cat([i.mvKeys2 for i in its], np.float32, 2), co, cat([i.mvMatches12 for i in its], np.int32, 2), cat([i.mK for i in its], np.float32, 9),
                                   [i.mSigma for i in its], ho, cat([i._pending for i in its], np.int32, 8))
        for i, t in zip(its, problem_tables(out, co, ho)):
            i._table, i._pending = t, None

    def table(self):
        if self._table is None:
            Initializer.evaluate_many([self])
        return self._table

    # ---- the reference's interface
    def result(self):
        """-> (success, R21 (3, 3), t21 (3, 1), vP3D (n1, 3), vbTriangulated[n1]) of the prepared pair; R21, t21 are None and the vectors empty where the reference leaves
        them so (false).  Fewer than 8 matches: false -- the reference's set drawing is undefined there, and Tracking.cc:954 asks for 100."""
        n1 = len(self.mvKeys1)
        none = (False, None, None, np.zeros((0, 3), np.float32), np.zeros(0, bool))
        if self._table is None and self._pending is None:
            raise CubeSlamError("Initializer: nothing prepared")
        T = self.table()
        c, _ = walk(T["model"], T["n_cand"], T["nGood"], T["cos_parallax"], T["n_inliers"])
        if c < 0:
            return none
        first = self.mvMatches12[:, 0]
        vP3D, vb = np.zeros((n1, 3), np.float32), np.zeros(n1, bool)
        vP3D[first] = T["points"][c]  # vP3D[vMatches12[i].first], :893
        vb[first] = mask_bits(T["good_mask"][c], T["N"])  # :897
        Rt = T["cand_Rt"][c]
        return True, Rt[:9].reshape(3, 3).copy(), Rt[9:].reshape(3, 1).copy(), vP3D, vb

    def Initialize(self, CurrentFrame_keys, vMatches12):
        self.prepare(CurrentFrame_keys, vMatches12)
        return self.result()
