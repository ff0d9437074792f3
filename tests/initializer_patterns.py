"""TEST INFRASTRUCTURE: seeded cases of the Initializer tests.  A case is one Initializer::Initialize call: the key points of the reference and of the current frame (x, y of
mvKeysUn; some of them unmatched, so that Normalize runs over more than the matches), vMatches12, K, sigma and the sets of eight its iterations draw (the partial Fisher-Yates
of Initializer.cc:83-98, ransac_draw<8> of csrc/ransac_batch.h, over a seeded RandomInt).  A scene is a cloud of points seen from two cameras, X2 = R X1 + t, up to `noise`
pixels; `outliers` of the matches are gross.

case(name) builds a case, judged(name) is the library's host path on it (ctx == NULL), computed once per case; CLAIMS says which branch of the reference each case is there for,
and tests/test_initializer_patterns.py checks that it is taken."""
import functools

import numpy as np

from cube_slam_amd import initializer as I
from cube_slam_amd._ransac import draw, offsets

F32 = np.float32
K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]], F32)


def _rot(axis, deg):
    a = np.asarray(axis, float); a = a / np.linalg.norm(a); t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def _project(X):
    return np.stack([500.0 * X[:, 0] / X[:, 2] + 320.0, 500.0 * X[:, 1] / X[:, 2] + 240.0], 1)


def scene(kind, N, seed, noise=0.3, outliers=0.0, far=0.0, tilt=(0.4, 0.2)):
    """-> keys1 (n1, 2), keys2 (n2, 2), vMatches12[n1], and the planted (R, t)."""
    rng = np.random.RandomState(seed)
    Rm, t = _rot([0.2, 1.0, 0.1], 3.0), np.array([0.5, 0.05, 0.02])
    z = rng.uniform(4.0, 8.0, N)
    x, y = rng.uniform(-0.5, 0.5, N) * z, rng.uniform(-0.4, 0.4, N) * z
    if kind == "plane":  # z = 6 + tilt . (x, y)
        x, y = rng.uniform(-2.5, 2.5, N), rng.uniform(-2.0, 2.0, N)
        z = 6.0 + tilt[0] * x + tilt[1] * y
    elif kind == "rotation":  # no translation: a homography whatever the depths
        Rm, t = _rot([0.1, 1.0, 0.0], 5.0), np.zeros(3)
    elif kind == "mixed":  # `far` of the points beyond the parallax of cos = 0.99998, the others near: CheckRT skips the depth tests of the far ones
        nfar = int(round(far * N))
        zf = rng.uniform(60.0, 120.0, N)
        isfar = np.zeros(N, bool); isfar[rng.permutation(N)[:nfar]] = True
        scale = np.where(isfar, zf / z, 1.0)
        x, y, z = x * scale, y * scale, z * scale
        t = np.array([0.3, 0.02, 0.0])
    X1 = np.stack([x, y, z], 1)
    X2 = X1 @ Rm.T + t
    uv1 = _project(X1) + rng.normal(size=(N, 2)) * noise
    uv2 = _project(X2) + rng.normal(size=(N, 2)) * noise
    if kind == "garbage":
        uv2 = np.stack([rng.uniform(20, 620, N), rng.uniform(20, 460, N)], 1)
    out = rng.rand(N) < outliers
    uvo = np.stack([rng.uniform(20, 620, N), rng.uniform(20, 460, N)], 1)
    near = np.linalg.norm(uvo - uv2, axis=1) < 40.0  # (a gross outlier stays gross)
    uvo[near, 0] = np.where(uv2[near, 0] < 320, uv2[near, 0] + 150.0, uv2[near, 0] - 150.0)
    uv2[out] = uvo[out]
    n1, n2 = N + N // 4 + 3, N + N // 5 + 2
    first, second = np.sort(rng.permutation(n1)[:N]), rng.permutation(n2)[:N]
    keys1 = np.stack([rng.uniform(20, 620, n1), rng.uniform(20, 460, n1)], 1)
    keys2 = np.stack([rng.uniform(20, 620, n2), rng.uniform(20, 460, n2)], 1)
    keys1[first], keys2[second] = uv1, uv2
    vMatches12 = np.full(n1, -1, np.int32); vMatches12[first] = second
    return {"keys1": keys1.astype(F32), "keys2": keys2.astype(F32), "vMatches12": vMatches12, "planted": (Rm, t), "planted_outlier": out}


# name: (scene kind, N, seed, hypotheses, sigma, keyword arguments of scene)
CASES = {
    "general": ("general", 130, 101, 24, 1.0, {}),                       # F chosen, success; more than 51 good points: vCosParallax[50]
    "plane": ("plane", 130, 500, 24, 1.0, {"tilt": (1.0, 0.0)}),      # H chosen, success: the second best candidate stays below 0.75 of the best
    "plane_d1d2": ("rotation", 64, 103, 6, 1.0, {"noise": 0.0}),        # H chosen, d1 / d2 < 1.00001: the return of :604
    "rotation": ("rotation", 65, 104, 12, 1.0, {"noise": 0.5}),          # H chosen, eight candidates, rejected on parallax
    "similar": ("mixed", 130, 403, 24, 1.0, {"far": 0.7, "noise": 0.7}),   # F chosen, two candidates above 0.7 maxGood: nsimilar > 1
    "outliers": ("general", 130, 302, 24, 1.0, {"outliers": 0.3}),       # 30 % gross outliers; no H hypothesis scores (SH = 0, RH = 0)
    "few": ("general", 31, 107, 12, 1.0, {}),                            # fewer than 51 good points: vCosParallax[nGood - 1]
    "no_model": ("garbage", 33, 108, 5, 1e-7, {}),                       # no hypothesis scores: no model
    "empty": ("general", 0, 109, 0, 1.0, {}),                            # no matches and no hypotheses: a hole in a batch
    "n8": ("general", 8, 110, 3, 1.0, {}),                               # the set is the whole problem
    "n32": ("general", 32, 111, 5, 1.0, {}), "n33": ("general", 33, 112, 5, 1.0, {}),  # the mask-word seam
    "redraw": ("general", 300, 5212, 3, 1.0, {"outliers": 0.2}),          # set 0: the first start vector of the 8 x 9 completion has nothing along the null space, OpenCV draws again
    "n63": ("general", 63, 113, 5, 1.0, {}), "n64": ("general", 64, 114, 5, 1.0, {}), "n65": ("general", 65, 115, 1, 1.0, {}),  # the lane-stride and ballot seams
}
# sets that are not the first H of the case's own stream: name -> (seed of the stream, sets drawn, those kept)
SETS = {"redraw": (9212, 44, [43, 0, 1])}
ALL = list(CASES)
# the branch each case is there for: the model and a word for tests/test_initializer_patterns.py
CLAIMS = {"general": ("F", "success idx50"), "plane": ("H", "success"), "plane_d1d2": ("H", ":604"), "rotation": ("H", "parallax"), "similar": ("F", "nsimilar"),
          "outliers": ("F", "SH0"), "few": ("F", "idx_last"), "no_model": ("none", ""), "empty": ("none", "")}
BATCHES = [["general"], ["n8", "empty", "plane", "redraw"], ["no_model", "few", "n33", "rotation", "n64"], ["plane_d1d2", "similar"], ["outliers", "n32", "n63", "n65"]]


@functools.lru_cache(maxsize=None)
def case(name):
    kind, N, seed, H, sigma, kw = CASES[name]
    c = scene(kind, N, seed, **kw)
    draw_seed, n_drawn, kept = SETS.get(name, (seed + 1000, H, list(range(H))))
    rng = np.random.RandomState(draw_seed)
    c.update(K=K, sigma=F32(sigma), N=N, sets=draw(N, 8, n_drawn, lambda a, b: int(rng.randint(a, b + 1)))[kept], name=name)
    first = np.nonzero(c["vMatches12"] >= 0)[0]
    c["matches"] = np.stack([first, c["vMatches12"][first]], 1).astype(np.int32)
    return c


def evaluate(cases, ctx=None):
    """cs_initializer_evaluate over a batch of cases -> (dict of the call's arrays, corr_off, hyp_off)."""
    co, ho = offsets(c["N"] for c in cases), offsets(len(c["sets"]) for c in cases)
    cat = lambda key, dt, w: np.concatenate([np.asarray(c[key], dt).reshape(-1, w) for c in cases])
    out = I.initializer_evaluate(ctx, offsets(len(c["keys1"]) for c in cases), cat("keys1", F32, 2), offsets(len(c["keys2"]) for c in cases), cat("keys2", F32, 2), co,
                                 cat("matches", np.int32, 2), cat("K", F32, 9), [c["sigma"] for c in cases], ho, cat("sets", np.int32, 8))
    return out, co, ho


@functools.lru_cache(maxsize=None)
def judged(name):
    """The host path on one case: the call's arrays (read-only)."""
    out, _, _ = evaluate([case(name)])
    for v in out.values():
        v.setflags(write=False)
    return out


KEYS = ("score", "matrix", "mask", "model", "best", "S", "RH", "n_inliers", "n_cand", "cand_Rt", "nGood", "cos_parallax", "good_mask", "points")


def concat(outs):
    """The arrays of several single-problem calls laid out as one batch's."""
    r = {}
    for k in KEYS:
        if k in ("score", "matrix", "mask"):
            r[k] = np.concatenate([o[k] for o in outs], axis=1)
        else:
            r[k] = np.concatenate([o[k] for o in outs], axis=0)
    return r


def raw_call(ctx, cases, sentinel=0x5A):
    """cs_initializer_evaluate called directly, every output byte set to `sentinel` beforehand -> (status, last error text, the output arrays): for the refusals, which must
    leave them untouched."""
    from cube_slam_amd._lib import lib, ptr
    co, ho = offsets(c["N"] for c in cases), offsets(len(c["sets"]) for c in cases)
    cat = lambda key, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(c[key], dt).reshape(-1, w) for c in cases])).reshape(-1)
    k1o, k2o = offsets(len(c["keys1"]) for c in cases), offsets(len(c["keys2"]) for c in cases)
    a1, a2, mt, k9, st = cat("keys1", F32, 2), cat("keys2", F32, 2), cat("matches", np.int32, 2), cat("K", F32, 9), cat("sets", np.int32, 8)
    sg = np.array([c["sigma"] for c in cases], F32)
    n, H, NC = len(cases), int(ho[-1]), int(co[-1])
    words = sum(len(c["sets"]) * ((c["N"] + 31) // 32) for c in cases)
    cwords = sum(8 * ((c["N"] + 31) // 32) for c in cases)
    sizes = (("score", F32, 2 * H), ("matrix", F32, 18 * H), ("mask", np.uint32, 2 * words), ("model", np.int32, n), ("best", np.int32, 2 * n), ("S", F32, 2 * n), ("RH", F32, n),
             ("n_inliers", np.int32, n), ("n_cand", np.int32, n), ("cand_Rt", F32, 96 * n), ("nGood", np.int32, 8 * n), ("cos_parallax", F32, 8 * n),
             ("good_mask", np.uint32, cwords), ("points", F32, 24 * NC))
    out = {k: np.frombuffer(bytes([sentinel]) * (np.dtype(dt).itemsize * max(sz, 1)), dt).copy() for k, dt, sz in sizes}
    cp = ctx.ptr if ctx is not None else None
    rc = lib().cs_initializer_evaluate(cp, n, ptr(k1o), ptr(a1), ptr(k2o), ptr(a2), ptr(co), ptr(mt), ptr(k9), ptr(sg), ptr(ho), ptr(st), *[ptr(out[k]) for k, _, _ in sizes])
    return rc, (lib().cs_last_error(cp).decode() if cp is not None else ""), out
