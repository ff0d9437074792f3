"""Judge of the Sim3 / relocalisation searches: a statement-by-statement numpy restatement of ORB_SLAM2::ORBmatcher::SearchByProjection(pKF, Scw, ...) (reference
orb_object_slam/src/ORBmatcher.cc:309-427), Fuse(pKF, Scw, ...) (:1010-1139), SearchBySim3 (:1141-1371) and SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
(:1727-1858) over flat arrays, and the generator of the map points the tests search with.  A helper, not a test module.

Every float operation is an explicit np.float32 step in the reference's association; a cv::Mat product is one gemm per row (double accumulation over k ascending, one rounding),
cv::norm and Mat::dot accumulate in double, 1 / z and 1.0 / z are a double division rounded to float.  log is libm's logf through ctypes (np.log on float32 is numpy's own routine).
Windows come through the oracle's GetFeaturesInArea and distances through its DescriptorDistance, both pinned to the reference elsewhere.

Where the reference is undefined -- MapPoint::PredictScale (MapPoint.cc:524-533) returns a level outside mvScaleFactors, or mfMaxDistance / dist is not a positive normal float -- the
point is dropped and counted (`outside`), as the device code does."""
import ctypes as C
import math

import numpy as np

from cube_slam_amd import synth

f32, f64 = np.float32, np.float64
TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30  # ORBmatcher.cc:42-44
W, H = 1241, 376
FX, FY, CX, CY = 721.5377, 721.5377, 609.5593, 172.854
BOUNDS = (0.0, float(W), 0.0, float(H))
SF = np.float32(1.2) ** np.arange(8, dtype=np.float32)
LOG_SF = float(np.float32(math.log(1.2)))  # mfLogScaleFactor = log(mfScaleFactor), stored as float (Frame.cc / KeyFrame.cc)

_libm = C.CDLL("libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def logf(x):
    return f32(_libm.logf(C.c_float(float(x))))


def gemm3(R, p, t):
    """cv::Mat R(3x3) * p(3x1) + t: cv::gemm, double accumulation over k ascending, (float)(s * alpha + t * beta) with alpha = beta = 1."""
    R = np.asarray(R, f32).reshape(9)
    out = np.zeros(3, f32)
    for r in range(3):
        s = f64(0)
        for k in range(3):
            s = s + f64(R[r * 3 + k]) * f64(p[k])
        out[r] = f32(s * f64(1.0) + f64(t[r]) * f64(1.0))
    return out


def norm3(v):
    s = f64(0)
    for k in range(3):
        s = s + f64(v[k]) * f64(v[k])
    return f32(np.sqrt(s))


def c_round(x):
    x = float(x)
    return math.floor(x + 0.5) if x >= 0 else math.ceil(x - 0.5)


def rot_bin(a1, a2):  # :1822-1827
    factor = f32(f32(1.0) / f32(HISTO_LENGTH))
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    b = c_round(f32(rot * factor))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes):  # :1860-1901
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < f32(f32(0.1) * f32(max1)):
        ind2 = ind3 = -1
    elif max3 < f32(f32(0.1) * f32(max1)):
        ind3 = -1
    return ind1, ind2, ind3


def predict_scale(max_distance, dist, log_sf, n_levels):
    """MapPoint::PredictScale; None where the reference is undefined."""
    with np.errstate(all="ignore"):
        ratio = f32(f32(max_distance) / f32(dist))
    if not (np.isfinite(ratio) and ratio >= np.finfo(f32).tiny):
        return None
    lf = math.ceil(f32(logf(ratio) / f32(log_sf)))
    return int(lf) if 0 <= lf < n_levels else None


SIM3, PAIR, RELOC = 0, 1, 2


def preamble(mode, p, normal, min_d, max_d, T, intr, bounds, log_sf, sf, th):
    """One map point up to the window: ("ok", u, v, L, radius) or (reason,).  T = (Rcw, tcw, Ow) or, for PAIR, (R1w, t1w, sR21, t21)."""
    fx, fy, cx, cy = [f32(a) for a in intr]
    minX, maxX, minY, maxY = [f32(b) for b in bounds]
    p = np.asarray(p, f32)
    with np.errstate(all="ignore"):
        pc = gemm3(T[0], p, T[1])
        if mode == PAIR:
            pc = gemm3(T[2], pc, T[3])
        if mode == RELOC:  # :1757-1767 -- no depth test, u = fx * xc * invzc + cx, the Frame's bounds with both ends inclusive
            xc, yc = pc[0], pc[1]
            invzc = f32(f64(1.0) / f64(pc[2]))
            u = f32(f32(f32(fx * xc) * invzc) + cx)
            v = f32(f32(f32(fy * yc) * invzc) + cy)
            if u < minX or u > maxX:
                return ("image",)
            if v < minY or v > maxY:
                return ("image",)
        else:  # :349-362, :1051-1064, :1202-1214
            if pc[2] < 0.0:
                return ("depth",)
            invz = f32(f64(1.0) / f64(pc[2]))
            x = f32(pc[0] * invz)
            y = f32(pc[1] * invz)
            u = f32(f32(fx * x) + cx)
            v = f32(f32(fy * y) + cy)
            if not (u >= minX and u < maxX and v >= minY and v < maxY):  # KeyFrame::IsInImage
                return ("image",)
        maxDistance = f32(f32(1.2) * f32(max_d))  # MapPoint::GetMaxDistanceInvariance
        minDistance = f32(f32(0.8) * f32(min_d))
        if mode == PAIR:
            PO = pc  # :1218: the camera-frame vector
        else:
            Ow = np.asarray(T[2], f32)
            PO = np.array([f32(p[0] - Ow[0]), f32(p[1] - Ow[1]), f32(p[2] - Ow[2])], f32)
        dist = norm3(PO)
        if dist < minDistance or dist > maxDistance:
            return ("range",)
        if mode == SIM3:  # :374-377
            dot = f64(0)
            for k in range(3):
                dot = dot + f64(PO[k]) * f64(f32(normal[k]))
            if dot < f64(0.5) * f64(dist):
                return ("angle",)
        L = predict_scale(max_d, dist, log_sf, len(sf))
        if L is None:
            return ("outside",)
        radius = f32(f32(th) * f32(sf[L]))
    return ("ok", u, v, L, radius)


def _count(stats, key):
    if stats is not None:
        stats[key] = stats.get(key, 0) + 1


def _best(oracle, F, keys_oct, desc, dMP, u, v, radius, L, lo_hi_in_area, blocked):
    """The candidate loop shared by the four functions: first strict minimum over the window, skipping `blocked` key points and levels outside [L - 1, L] unless the window call
    already filtered the levels (relocalisation)."""
    if lo_hi_in_area:
        idxs = oracle.get_features_in_area(F, u, v, radius, L - 1, L + 1)
    else:
        idxs = oracle.get_features_in_area(F, u, v, radius)
    bestDist, bestIdx = 2 ** 31 - 1, -1
    for idx in idxs:
        idx = int(idx)
        if blocked[idx]:
            continue
        if not lo_hi_in_area and (keys_oct[idx] < L - 1 or keys_oct[idx] > L):
            continue
        d = oracle.descriptor_distance(dMP, desc[idx])
        if d < bestDist:
            bestDist, bestIdx = d, idx
    return bestIdx, bestDist


def _claim_search(oracle, mode, frame, T, pts, intr, log_sf, sf, th, accept, train_blocked, kf_angle=None, check_orientation=False, stats=None):
    keys, desc, F = frame[:3]
    N = len(keys)
    octv = keys["octave"]
    held = np.zeros(N, bool) if train_blocked is None else (np.asarray(train_blocked) != 0)
    held = held.copy()
    match = np.full(N, -1, np.int32)
    nmatches, outside = 0, 0
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    wanted = {}
    for i in range(len(pts["skip"])):
        if pts["skip"][i]:
            _count(stats, "skip")
            continue
        res = preamble(mode, pts["world_pos"][i], pts["normal"][i] if mode == SIM3 else None, pts["min_distance"][i], pts["max_distance"][i], T, intr, BOUNDS if frame[3] is None else frame[3],
                       log_sf, sf, th)
        if res[0] != "ok":
            _count(stats, res[0])
            outside += res[0] == "outside"
            continue
        _, u, v, L, radius = res
        if stats is not None:  # what the point would take if no earlier point of this call had claimed anything
            b0 = np.zeros(N, bool) if train_blocked is None else (np.asarray(train_blocked) != 0)
            wi, wd = _best(oracle, F, octv, desc, pts["mp_desc"][i], u, v, radius, L, mode == RELOC, b0)
            if wi >= 0 and wd <= accept:
                wanted[wi] = wanted.get(wi, 0) + 1
        bestIdx, bestDist = _best(oracle, F, octv, desc, pts["mp_desc"][i], u, v, radius, L, mode == RELOC, held)
        if bestIdx >= 0 and bestDist < 256 and bestDist <= accept:  # (:392, :1792 start at 256)
            held[bestIdx] = True
            match[bestIdx] = i
            nmatches += 1
            if check_orientation:
                rotHist[rot_bin(kf_angle[i], keys["angle"][bestIdx])].append(bestIdx)
    n_cut = 0
    if check_orientation:  # :1836-1855
        ind = three_maxima([len(h) for h in rotHist])
        for b in range(HISTO_LENGTH):
            if b not in ind:
                for idx in rotHist[b]:
                    match[idx] = -1
                    nmatches -= 1
                    n_cut += 1
    if stats is not None:
        stats["cut"] = n_cut
        stats["contested"] = sum(1 for c in wanted.values() if c >= 2)
    return match, nmatches, outside


def make_frame(oracle, keys, desc, bounds=None):
    return (keys, desc, oracle.make_frame(keys, desc, BOUNDS if bounds is None else bounds), bounds)


def search_by_projection_reloc(oracle, frame, Rcw, tcw, Ow, pts, kf_angle, intr, log_sf, sf, th, orb_dist, check_orientation, train_blocked=None, stats=None):
    """:1727-1858 -> (train_match per key point of the current frame, nmatches, outside)."""
    return _claim_search(oracle, RELOC, frame, (Rcw, tcw, Ow), pts, intr, log_sf, sf, th, orb_dist, train_blocked, kf_angle, check_orientation, stats)


def search_by_projection_sim3(oracle, frame, Rcw, tcw, Ow, pts, intr, log_sf, sf, th, train_blocked=None, stats=None):
    """:309-427 -> (train_match per key point of the key frame, nmatches, outside)."""
    return _claim_search(oracle, SIM3, frame, (Rcw, tcw, Ow), pts, intr, log_sf, sf, th, TH_LOW, train_blocked, None, False, stats)


def _independent(oracle, mode, frame, T, pts, intr, log_sf, sf, th, train_blocked, stats):
    keys, desc, F = frame[:3]
    n = len(pts["skip"])
    blocked = np.zeros(len(keys), bool) if train_blocked is None else (np.asarray(train_blocked) != 0)
    bi = np.full(n, -1, np.int32)
    bd = np.full(n, 2 ** 31 - 1, np.int32)  # INT_MAX (:1096, :1238)
    outside = 0
    for i in range(n):
        if pts["skip"][i]:
            _count(stats, "skip")
            continue
        res = preamble(mode, pts["world_pos"][i], pts["normal"][i] if mode == SIM3 else None, pts["min_distance"][i], pts["max_distance"][i], T, intr, BOUNDS if frame[3] is None else frame[3],
                       log_sf, sf, th)
        if res[0] != "ok":
            _count(stats, res[0])
            outside += res[0] == "outside"
            continue
        _, u, v, L, radius = res
        bi[i], bd[i] = _best(oracle, F, keys["octave"], desc, pts["mp_desc"][i], u, v, radius, L, False, blocked)
    return bi, bd, outside


def fuse_sim3(oracle, frame, Rcw, tcw, Ow, pts, intr, log_sf, sf, th, train_blocked=None, stats=None):
    """:1010-1139, the search -> (best_idx, best_dist, nFused, outside)."""
    bi, bd, outside = _independent(oracle, SIM3, frame, (Rcw, tcw, Ow), pts, intr, log_sf, sf, th, train_blocked, stats)
    return bi, bd, int((bd <= TH_LOW).sum()), outside


def search_by_sim3(oracle, frame1, frame2, R1w, t1w, R2w, t2w, sR12, t12, sR21, t21, pts1, pts2, intr, log_sf, sf, th, train_blocked1=None, train_blocked2=None, stats=None):
    """:1141-1371 -> (matches12 per key point of KF1, nFound, outside)."""
    s1 = None if stats is None else {}
    s2 = None if stats is None else {}
    bi1, bd1, o1 = _independent(oracle, PAIR, frame2, (R1w, t1w, sR21, t21), pts1, intr, log_sf, sf, th, train_blocked2, s1)
    bi2, bd2, o2 = _independent(oracle, PAIR, frame1, (R2w, t2w, sR12, t12), pts2, intr, log_sf, sf, th, train_blocked1, s2)
    vnMatch1 = np.where(bd1 <= TH_HIGH, bi1, -1)
    vnMatch2 = np.where(bd2 <= TH_HIGH, bi2, -1)
    m12 = np.full(len(vnMatch1), -1, np.int32)
    nFound = 0
    for i1 in range(len(vnMatch1)):  # :1353-1368
        idx2 = int(vnMatch1[i1])
        if idx2 >= 0 and idx2 < len(vnMatch2) and vnMatch2[idx2] == i1:
            m12[i1] = idx2
            nFound += 1
    if stats is not None:
        for k in set(s1) | set(s2):
            stats[k] = s1.get(k, 0) + s2.get(k, 0)
    return m12, nFound, o1 + o2


# ------------------------------------------------------------------------------------------------------------------------------ inputs of the tests
def frames(oracle):
    """The frame pair of tests/test_match_gpu.py: 1241 x 376, 2 000 features, the texture shifted by 4 px."""
    e = oracle.ORBextractor(2000, 1.2, 8, 20, 7)
    return [e(synth.texture_image(77, W, H, shift=4 * i)) for i in range(2)]


def small_pose(seed, x_only=False):
    """A camera pose with a small rotation and translation: (Rcw[9], tcw[3], Ow[3]) in float32; Ow = -Rcw.t() * tcw as one gemm.  x_only: a rotation about the x axis -- its
    first row is (1, 0, 0), so the reference's scw = sqrt(sRcw.row(0).dot(sRcw.row(0))) of Scw = [s R | s t] is exactly s and, for s a power of two, its Rcw = sRcw / scw and
    tcw are exactly R and t under any reading of the scalar cv::MatExpr operations."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-0.03, 0.03, 3)
    if x_only:
        w[1] = w[2] = 0.0
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / a
    R = (np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K).astype(f32)
    t = rng.uniform(-0.3, 0.3, 3).astype(f32)
    Ow = gemm3(-R.T.copy(), t, np.zeros(3, f32))
    return R.reshape(9).copy(), t, Ow


FRACTIONS = ("j1", "behind", "out_of_image", "range", "angle", "skip", "outside", "twin")


def map_points(keys, desc, dx, T, seed, frac=0.05, angle_test=True, dist_of=None):
    """Key points back-projected at depths 4 - 40 into the camera frame of the search (shifted by dx pixels: where the other frame sees the same texture) and taken to the world
    through T = (Rcw, tcw, Ow).  max_distance = depth * SF[octave] * j, j uniform in (1 / 1.2, 1]: the predicted level is the key point's octave for most points;
    min_distance = max_distance / SF[7]; normal = unit(p - Ow) + noise.  A seeded fraction `frac` of the points each: j = 1 exactly, behind the camera, out of the image, dist
    outside the range, viewing angle past 60 degrees, skip set, predicted level outside the table, and a twin of the point before it (the same landmark held twice in the map,
    three descriptor bits flipped: the two compete for one key point).  dist_of(pc, p): the distance the search measures (default |p - Ow|)."""
    rng = np.random.default_rng(seed)
    n = len(keys)
    A = np.asarray(T[0], f64).reshape(3, 3)  # camera = A p + t (a rotation, or a rotation times a scale)
    t = np.asarray(T[1], f64)
    Ow = np.asarray(T[2], f64)
    pick = {k: rng.uniform(size=n) < frac for k in FRACTIONS}
    d = rng.uniform(4, 40, n)
    x = keys["x"].astype(f64) + dx + rng.normal(0, 1.5, n)  # (pixel noise: the window radius matters)
    y = keys["y"].astype(f64) + rng.normal(0, 1.5, n)
    x = np.where(pick["out_of_image"], np.where(rng.uniform(size=n) < 0.5, -60.0 - x, W + 60.0 + x), x)
    pc = np.stack([(x - CX) / FX * d, (y - CY) / FY * d, d], axis=1)
    pc[pick["behind"]] *= -1.0
    p = np.linalg.solve(A, (pc - t).T).T.astype(f32)
    dist = np.linalg.norm(p.astype(f64) - Ow, axis=1) if dist_of is None else dist_of(pc, p)
    j = np.where(pick["j1"], 1.0, 1.0 - rng.uniform(size=n) * (1.0 - 1.0 / 1.2))
    maxd = (d.astype(f32) * SF[np.clip(keys["octave"], 0, 7)] * j.astype(f32)).astype(f32)
    far = pick["range"] & (rng.uniform(size=n) < 0.5)
    maxd = np.where(far, dist * 0.7, maxd).astype(f32)  # dist > 1.2 max
    maxd = np.where(pick["outside"], dist * float(SF[7]) * rng.uniform(1.02, 1.24, n), maxd).astype(f32)  # level n_levels or n_levels + 1, inside 0.8 min <= dist
    mind = (maxd / SF[7]).astype(f32)
    mind = np.where(pick["range"] & ~far, dist * 1.5, mind).astype(f32)  # dist < 0.8 min
    po = p.astype(f64) - Ow
    nrm = po / np.linalg.norm(po, axis=1, keepdims=True) + rng.normal(0, 0.05, (n, 3))
    if angle_test:
        side = np.cross(po, [0.0, 1.0, 0.0])
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        tilt = np.radians(rng.uniform(65, 110, n))[:, None]
        nrm = np.where(pick["angle"][:, None], np.cos(tilt) * po / np.linalg.norm(po, axis=1, keepdims=True) + np.sin(tilt) * side, nrm)
    desc = np.array(desc, np.uint8)
    p, nrm = np.ascontiguousarray(p, f32), np.ascontiguousarray(nrm, f32)
    for i in np.nonzero(pick["twin"])[0]:
        if i == 0:
            continue
        p[i], nrm[i], mind[i], maxd[i], desc[i] = p[i - 1], nrm[i - 1], mind[i - 1], maxd[i - 1], desc[i - 1]
        for b in rng.integers(0, 256, 3):
            desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return {"world_pos": p, "normal": nrm, "min_distance": mind, "max_distance": maxd, "skip": pick["skip"].astype(np.uint8), "mp_desc": desc}


def blocked_split(n, seed, pre_matched=0.05, dynamic=0.05):
    """Per key point of a searched frame: (holds a map point from before the call, !KeysStatic)."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=n) < pre_matched).astype(np.uint8), (rng.uniform(size=n) < dynamic).astype(np.uint8)


def blocked_keys(n, seed, pre_matched=0.05, dynamic=0.05):
    """train_blocked of a searched frame: a map point from before the call || !KeysStatic."""
    pre, dyn = blocked_split(n, seed, pre_matched, dynamic)
    return pre | dyn


def all_outside(pts, dist):
    """Every point at a predicted level of n_levels: max_distance = 1.1 * SF[7] * dist, dist = what the search measures (camera_dist)."""
    out = dict(pts)
    out["max_distance"] = (dist * float(SF[7]) * 1.1).astype(f32)
    out["min_distance"] = (out["max_distance"] / SF[7]).astype(f32)
    out["skip"] = np.zeros(len(dist), np.uint8)
    return out


def camera_dist(p, *Rt):
    """|R_n (... (R_1 p + t_1) ...) + t_n| in double; camera_dist(p, I, -Ow) = |p - Ow|."""
    q = np.asarray(p, f64)
    for k in range(0, len(Rt), 2):
        q = q @ np.asarray(Rt[k], f64).reshape(3, 3).T + np.asarray(Rt[k + 1], f64)
    return np.linalg.norm(q, axis=1)


def projection_case(fr, seed, pre_matched=0.05):
    """Map points from frame 1's key points, searched in frame 2 through a small pose: (T = (Rcw, tcw, Ow), points, train_blocked of frame 2)."""
    (k1, d1), (k2, d2) = fr
    T = small_pose(seed, x_only=True)
    return T, map_points(k1, d1, -4.0, T, seed + 1), blocked_keys(len(k2), seed + 2, pre_matched)


def rotated_angles(angle, seed):
    """The key-frame angles with a seeded per-point offset on 30 % of the points: their claims fall into other bins of the rotation histogram."""
    rng = np.random.default_rng(seed)
    off = np.where(rng.uniform(size=len(angle)) < 0.3, rng.uniform(40, 320, len(angle)), 0.0)
    return np.mod(angle.astype(f64) + off, 360.0).astype(f32)


def sim3_case(fr, seed, s12):
    """Two key frames in worlds that differ by the similarity (s12, R12, t12), s12 in {1, 2, 0.5} so that s12 * R12 and (1.0 / s12) * R12.t() are exact under any reading: the eight
    transforms of cs_match_by_sim3 in its order, the points of both sides (KF1's are seen by KF2 where frame 2 shows the texture, and the other way round) and the blocked key points."""
    (k1, d1), (k2, d2) = fr
    R1w, t1w, _ = small_pose(seed)
    R2w, t2w, _ = small_pose(seed + 1)
    R12, t12, _ = small_pose(seed + 2)
    sR12 = (f32(s12) * R12).astype(f32)
    sR21 = (f32(1.0 / s12) * R12.reshape(3, 3).T.reshape(9)).astype(f32)
    t21 = gemm3(-sR21, t12, np.zeros(3, f32))
    z3 = np.zeros(3)
    m = lambda a: np.asarray(a, f64).reshape(3, 3)
    cam = lambda pc, p: np.linalg.norm(pc, axis=1)
    A1, b1 = m(sR21) @ m(R1w), m(sR21) @ t1w.astype(f64) + t21  # camera 2 = A1 p + b1 for a point of KF1's world
    A2, b2 = m(sR12) @ m(R2w), m(sR12) @ t2w.astype(f64) + t12
    pts1 = map_points(k1, d1, -4.0, (A1, b1, z3), seed + 3, angle_test=False, dist_of=cam)
    pts2 = map_points(k2, d2, 4.0, (A2, b2, z3), seed + 4, angle_test=False, dist_of=cam)
    return (R1w, t1w, R2w, t2w, sR12, t12, sR21, t21), pts1, pts2, blocked_keys(len(k1), seed + 5, 0.0), blocked_keys(len(k2), seed + 6, 0.0)


def points_tuple(pts):
    return (pts["world_pos"], pts["min_distance"], pts["max_distance"], pts["skip"], pts["mp_desc"])
