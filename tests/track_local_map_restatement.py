"""Judge of the TrackLocalMap entries: a statement-by-statement numpy restatement of Frame::isInFrustum (reference orb_object_slam/src/Frame.cc:346-402),
Tracking::SearchLocalPoints (Tracking.cc:2673-2728) with ORBmatcher::SearchByProjection(F, vpMapPoints, th) and RadiusByViewingCos (ORBmatcher.cc:50-150),
Tracking::UpdateLocalPoints (:2740-2764), Tracking::UpdateLocalKeyFrames (:2766-2874), the preamble of ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:871-920) and the
chain Tracking::TrackLocalMap (:1356-1416) over flat arrays, and the generators of what the tests run them on.  A helper, not a test module.

The float primitives are those of tests/sim3_restatement.py (every float operation an explicit np.float32 step in the reference's association; a cv::Mat product one gemm per row;
cv::norm and Mat::dot accumulated in double; libm's logf).  Windows come through the oracle's GetFeaturesInArea, pinned to the reference elsewhere.

Two places where the reference is undefined are decided as the device code decides them: a predicted level outside mvScaleFactors drops the point and counts it (`outside`), and a
projection that is not finite (PcZ == 0: NaN passes every comparison of the bounds test) rejects it.

The std::map<KeyFrame *, int> of UpdateLocalKeyFrames is walked in ascending index of the key-frame table: the order the library defines for it."""
import math

import numpy as np

from tests.sim3_restatement import BOUNDS, CX, CY, FX, FY, LOG_SF, SF, TH_HIGH, TH_LOW, f32, f64, gemm3, logf, norm3, predict_scale  # noqa: F401
from tests import sim3_restatement as S

BF = 386.1448
INTR = (FX, FY, CX, CY, BF)
POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)
REJECTS = ("skip", "depth", "image", "range", "angle", "outside")


def is_in_frustum(p, normal, min_d, max_d, Rcw, tcw, Ow, intr, bounds, log_sf, n_levels, viewing_cos_limit=0.5):
    """Frame.cc:346-402 -> ("ok", u, v, uR, L, viewCos) or (reason,)."""
    fx, fy, cx, cy, bf = [f32(a) for a in intr]
    minX, maxX, minY, maxY = [f32(b) for b in bounds]
    p = np.asarray(p, f32)
    with np.errstate(all="ignore"):
        Pc = gemm3(Rcw, p, tcw)
        PcX, PcY, PcZ = Pc[0], Pc[1], Pc[2]
        if PcZ < f32(0.0):
            return ("depth",)
        invz = f32(f32(1.0) / PcZ)
        u = f32(f32(f32(fx * PcX) * invz) + cx)
        v = f32(f32(f32(fy * PcY) * invz) + cy)
        if not (np.isfinite(u) and np.isfinite(v)):  # (the second deviation)
            return ("image",)
        if u < minX or u > maxX:
            return ("image",)
        if v < minY or v > maxY:
            return ("image",)
        maxDistance = f32(f32(1.2) * f32(max_d))
        minDistance = f32(f32(0.8) * f32(min_d))
        Ow = np.asarray(Ow, f32)
        PO = np.array([f32(p[0] - Ow[0]), f32(p[1] - Ow[1]), f32(p[2] - Ow[2])], f32)
        dist = norm3(PO)
        if dist < minDistance or dist > maxDistance:
            return ("range",)
        dot = f64(0)
        for k in range(3):
            dot = dot + f64(PO[k]) * f64(f32(normal[k]))
        viewCos = f32(dot / f64(dist))  # PO.dot(Pn) is a double, dist converts to double: one division, one rounding
        if viewCos < f32(viewing_cos_limit):
            return ("angle",)
        L = predict_scale(max_d, dist, log_sf, n_levels)
        if L is None:
            return ("outside",)
        uR = f32(u - f32(bf * invz))
    return ("ok", u, v, uR, L, viewCos)


def radius_by_viewing_cos(viewCos):
    """ORBmatcher.cc:144-150: the float against the double literal 0.998."""
    return f32(2.5) if f64(f32(viewCos)) > f64(0.998) else f32(4.0)


def frustum_all(pts, Rcw, tcw, Ow, intr, bounds, log_sf, n_levels, limit=0.5):
    """isInFrustum for every point that is not skipped: the per-point fields (zeros / level -1 where not in view) and the reason of every rejection."""
    n = len(pts["skip"])
    out = {"in_view": np.zeros(n, np.uint8), "proj": np.zeros((n, 3), f32), "pred_level": np.full(n, -1, np.int32), "view_cos": np.zeros(n, f32), "reason": ["skip"] * n}
    for i in range(n):
        if pts["skip"][i]:
            continue
        r = is_in_frustum(pts["world_pos"][i], pts["normal"][i], pts["min_distance"][i], pts["max_distance"][i], Rcw, tcw, Ow, intr, bounds, log_sf, n_levels, limit)
        out["reason"][i] = r[0]
        if r[0] == "ok":
            out["in_view"][i] = 1
            out["proj"][i] = (r[1], r[2], r[3])
            out["pred_level"][i] = r[4]
            out["view_cos"][i] = r[5]
    return out


def search_local_points(oracle, frame, Rcw, tcw, Ow, pts, blocks, intr, bounds, log_sf, sf, th, nnratio=0.8, train_blocked=None, limit=0.5, stats=None, fr=None):
    """Tracking.cc:2696-2727 -> the dict ORBmatcher.SearchLocalPoints returns.  fr: the frustum fields when the caller has them already."""
    if fr is None:
        fr = frustum_all(pts, Rcw, tcw, Ow, intr, bounds, log_sf, len(sf), limit)
    N = len(frame[0])
    n_to_match = int(fr["in_view"].sum())
    out = {k: fr[k] for k in ("in_view", "proj", "pred_level", "view_cos")}
    out["n_to_match"] = n_to_match
    out["outside"] = sum(1 for r in fr["reason"] if r == "outside")
    if stats is not None:
        for r in fr["reason"]:
            if r != "ok":
                stats[r] = stats.get(r, 0) + 1
    tm, nm = np.full(N, -1, np.int32), 0
    if n_to_match > 0:  # :2717
        tm, nm = search_by_projection(oracle, frame, fr, blocks, pts["mp_desc"], sf, th, nnratio, train_blocked, stats)
    out["train_match"], out["nmatches"] = tm, nm
    return out


def search_by_projection(oracle, frame, fr, blocks, mp_desc, sf, th, nnratio, train_blocked=None, stats=None):
    """ORBmatcher.cc:50-142 over the fields isInFrustum left (fr) -> (train_match, nmatches).  frame = sim3_restatement.make_frame(...).  A key point is skipped when it holds a
    map point with observations -- from before the call (train_blocked, which also carries !KeysStatic) or claimed in this call by a point with blocks set.  The return value is the
    reference's: nmatches++ per assignment (:137), so a key point taken over by a later point counts twice."""
    log = []
    tm = _search_logged(oracle, frame, fr, blocks, mp_desc, sf, th, nnratio, train_blocked, stats, log)
    return tm, len(log)


def _search_logged(oracle, frame, fr, blocks, mp_desc, sf, th, nnratio, train_blocked, stats, log):
    keys, desc, F = frame[:3]
    N = len(keys)
    octv = keys["octave"]
    never = np.zeros(N, bool) if train_blocked is None else (np.asarray(train_blocked) != 0)
    holder = np.full(N, -1, np.int64)
    bFactor = f32(th) != 1.0
    wanted = {}
    n_r = {2.5: 0, 4.0: 0}
    for i in range(len(fr["in_view"])):
        if not fr["in_view"][i]:
            continue
        L = int(fr["pred_level"][i])
        r = radius_by_viewing_cos(fr["view_cos"][i])
        n_r[float(r)] += 1
        if bFactor:
            r = f32(r * f32(th))
        idxs = np.asarray(oracle.get_features_in_area(F, fr["proj"][i, 0], fr["proj"][i, 1], f32(r * f32(sf[L])), L - 1, L), np.int64)
        if len(idxs) == 0:
            continue
        dists = POP[desc[idxs] ^ mp_desc[i]].sum(1)
        if stats is not None:
            ok0 = ~never[idxs]
            if ok0.any() and dists[ok0].min() <= TH_HIGH:
                j = int(idxs[ok0][np.argmin(dists[ok0])])
                wanted[j] = wanted.get(j, 0) + 1
        bestDist = bestDist2 = 256
        bestLevel = bestLevel2 = bestIdx = -1
        for idx, dist in zip(idxs, dists):
            if never[idx] or (holder[idx] >= 0 and blocks[holder[idx]]):  # :96-102
                continue
            if dist < bestDist:
                bestDist2, bestDist = bestDist, dist
                bestLevel2, bestLevel = bestLevel, octv[idx]
                bestIdx = idx
            elif dist < bestDist2:
                bestLevel2, bestDist2 = octv[idx], dist
        if bestDist <= TH_HIGH:
            if bestLevel == bestLevel2 and f32(bestDist) > f32(f32(nnratio) * f32(bestDist2)):
                continue
            holder[bestIdx] = i
            log.append((i, int(bestIdx)))
    if stats is not None:
        stats["contested"] = sum(1 for c in wanted.values() if c >= 2)
        stats["radius"] = n_r
    return holder.astype(np.int32)


def update_local_points(kf_off, kf_mp, skip):
    """Tracking.cc:2740-2764 over the lists of the local key frames in order."""
    seen = set()
    out = []
    for j in range(len(kf_off) - 1):
        for e in range(kf_off[j], kf_off[j + 1]):
            mp = int(kf_mp[e])
            if mp < 0:
                continue
            if mp in seen:  # mnTrackReferenceForFrame == mCurrentFrame.mnId
                continue
            if not skip[mp]:
                out.append(mp)
                seen.add(mp)
    return np.asarray(out, np.int32)


def update_local_keyframes(frame_mp, mp_skip, obs_off, obs_kf, kf_bad, cov_off, cov_kf, child_off, child_kf, parent):
    """Tracking.cc:2766-2874 -> (mvpLocalKeyFrames or None when no key frame received a vote, pKFmax or -1)."""
    counter = {}
    for mp in frame_mp:
        if mp < 0 or mp_skip[mp]:
            continue
        for o in range(obs_off[mp], obs_off[mp + 1]):
            counter[int(obs_kf[o])] = counter.get(int(obs_kf[o]), 0) + 1
    if not counter:
        return None, -1
    mx, kfmax = 0, -1
    local, mark = [], set()
    for kf in sorted(counter):  # the map's order: ascending index
        if kf_bad[kf]:
            continue
        if counter[kf] > mx:
            mx, kfmax = counter[kf], kf
        local.append(kf)
        mark.add(kf)
    for kf in list(local):  # the end iterator is taken before the pushes
        if len(local) > 80:
            break
        for nb in cov_kf[cov_off[kf]:cov_off[kf + 1]][:10]:
            if not kf_bad[nb] and int(nb) not in mark:
                local.append(int(nb)); mark.add(int(nb))
                break
        for ch in child_kf[child_off[kf]:child_off[kf + 1]]:
            if not kf_bad[ch] and int(ch) not in mark:
                local.append(int(ch)); mark.add(int(ch))
                break
        pa = int(parent[kf])
        if pa >= 0 and pa not in mark:
            local.append(pa); mark.add(pa)
            break  # leaves the outer loop
    return np.asarray(local, np.int32), kfmax


def fuse_preamble(pts, Rcw, tcw, Ow, intr, bounds, log_sf, n_levels):
    """ORBmatcher.cc:871-917 -> (uv, ur, pred_level, valid, outside): what cs_match_fuse takes from its caller."""
    fx, fy, cx, cy, bf = [f32(a) for a in intr]
    n = len(pts["skip"])
    uv, ur, lv, va = np.zeros((n, 2), f32), np.zeros(n, f32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    outside = 0
    for i in range(n):
        if pts["skip"][i]:
            continue
        r = S.preamble(S.SIM3, pts["world_pos"][i], pts["normal"][i], pts["min_distance"][i], pts["max_distance"][i], (Rcw, tcw, Ow), intr[:4], bounds, log_sf, np.ones(n_levels, f32), 1.0)
        if r[0] != "ok":
            outside += r[0] == "outside"
            continue
        with np.errstate(all="ignore"):
            pc = gemm3(Rcw, np.asarray(pts["world_pos"][i], f32), tcw)
            invz = f32(f64(1.0) / f64(pc[2]))
            uv[i] = (r[1], r[2]); ur[i] = f32(r[1] - f32(bf * invz)); lv[i] = r[3]; va[i] = 1
    return uv, ur, lv, va, outside


# ------------------------------------------------------------------------------------------------------------------------------ inputs of the tests
def local_points(frames, seed, n=3000):
    """n local map points seen by frame 0 through a small pose: two seeded sets of sim3_restatement.map_points over its key points (the second set holds every landmark again with other
    noise: points compete), with every reject class.  -> (T, pts, blocks, train_blocked)."""
    k, d = frames[0]
    T = S.small_pose(seed)
    a = S.map_points(k, d, 0.0, T, seed + 1)
    b = S.map_points(k, d, 0.0, T, seed + 2)
    pts = {key: np.concatenate([a[key], b[key]])[:n] for key in a}
    rng = np.random.default_rng(seed + 3)
    blocks = (rng.uniform(size=len(pts["skip"])) < 0.8).astype(np.uint8)
    return T, pts, blocks, S.blocked_keys(len(k), seed + 4, 0.1, 0.05)


EX_INTR = (512.0, 512.0, 320.0, 240.0, 40.0)
EX_BOUNDS = (0.0, 640.0, 0.0, 480.0)
EX_POSE = (np.eye(3, dtype=f32).reshape(9), np.zeros(3, f32), np.zeros(3, f32))


def exact_cases():
    """Points on the edges of every test of isInFrustum, with representable numbers: camera at the origin, fx = fy = 512, cx = 320, cy = 240, PcZ = 1.  Two set-ups: scale factor 2
    with 4 levels, and scale factor 1.1 with 8 levels (a level of -1 inside 0.8 min <= dist <= 1.2 max needs a scale factor below 1.2).  -> list of (name, log_sf, sf, pts, want)
    with want[i] = (in_view, level or None, radius or None)."""
    def pts_of(rows):
        n = len(rows)
        p = {"world_pos": np.zeros((n, 3), f32), "normal": np.zeros((n, 3), f32), "min_distance": np.zeros(n, f32), "max_distance": np.zeros(n, f32), "skip": np.zeros(n, np.uint8),
             "mp_desc": np.zeros((n, 32), np.uint8)}
        for i, (wp, nr, mn, mx) in enumerate(rows):
            p["world_pos"][i], p["normal"][i], p["min_distance"][i], p["max_distance"][i] = wp, nr, mn, mx
        return p
    z1 = (0.0, 0.0, 1.0)
    c998 = float(f32(0.998))
    two = [  # (world_pos, normal, mfMinDistance, mfMaxDistance), dist = |p|
        ((-0.625, 0.0, 1.0), (-0.625, 0.0, 1.0), 0.1, 1.0),     # u == mnMinX = 0
        ((0.625, 0.0, 1.0), (0.625, 0.0, 1.0), 0.1, 1.0),       # u == mnMaxX = 640
        ((0.0, -0.46875, 1.0), (0.0, 0.0, 1.0), 0.1, 1.0),      # v == mnMinY = 0
        ((0.0, 0.46875, 1.0), (0.0, 0.0, 1.0), 0.1, 1.0),       # v == mnMaxY = 480
        ((0.0, 0.0, 4.0), z1, 5.0, 4.0),                        # dist == 0.8f * 5 (rounds to 4)
        ((0.0, 0.0, float(f32(1.2))), z1, 0.1, 1.0),            # dist == 1.2f * 1
        (z1, (0.5, 0.5, 0.5), 0.1, 1.0),                        # viewCos == 0.5
        (z1, (0.0, 0.0, c998), 0.1, 1.0),                       # viewCos == float(0.998) > 0.998: radius 2.5
        (z1, (0.0, 0.0, 0.9979999), 0.1, 1.0),                  # just below: 4.0
        (z1, z1, 0.1, 1.0),                                     # level 0
        (z1, z1, 0.1, 0.9 * 8.0),                               # level 3 = n_levels - 1
        (z1, z1, 0.1, 0.9 * 16.0),                              # level 4 = n_levels: dropped
        ((0.0, 0.0, 0.0), z1, 0.0, 1.0),                        # PcZ == 0 and PcX == PcY == 0: u = v = NaN
        ((0.0, 0.0, -1.0), (0.0, 0.0, -1.0), 0.1, 1.0),         # behind
        ((-0.627, 0.0, 1.0), z1, 0.1, 1.0),                     # just left of the image
    ]
    want_two = [(1, 0, 2.5), (1, 0, 2.5), (1, 0, 4.0), (1, 0, 4.0), (1, 0, 2.5), (1, 0, 2.5), (1, 0, 4.0), (1, 0, 2.5), (1, 0, 4.0), (1, 0, 2.5), (1, 3, 2.5), (0, None, None), (0, None, None),
                (0, None, None), (0, None, None)]
    small = [
        (z1, z1, 0.1, 1.0 / 1.15),          # level -1: dropped
        (z1, z1, 0.1, 1.0),                 # level 0
        (z1, z1, 0.1, 0.98 * 1.1 ** 7),     # level 7
        (z1, z1, 0.1, 0.98 * 1.1 ** 8),     # level 8 = n_levels: dropped
    ]
    want_small = [(0, None, None), (1, 0, 2.5), (1, 7, 2.5), (0, None, None)]
    sf2 = f32(2.0) ** np.arange(4, dtype=f32)
    sf11 = f32(1.1) ** np.arange(8, dtype=f32)
    return [("sf2", float(f32(math.log(2.0))), sf2, pts_of(two), want_two), ("sf1.1", float(f32(math.log(1.1))), sf11, pts_of(small), want_small)]


def keyframe_lists(n_kf, n_points, per_kf, seed, none_frac=0.2):
    """CSR of key-frame map-point lists: per_kf entries each, a fraction -1, the rest seeded indices into a table of n_points."""
    rng = np.random.default_rng(seed)
    mp = rng.integers(0, max(n_points, 1), n_kf * per_kf).astype(np.int32)
    mp[rng.uniform(size=len(mp)) < none_frac] = -1
    return (np.arange(n_kf + 1) * per_kf).astype(np.int32), mp


def csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    for i, l in enumerate(lists):
        off[i + 1] = off[i] + len(l)
    flat = np.asarray([x for l in lists for x in l], np.int32)
    return off, flat


def graph_case(name):
    """Key-frame graphs for UpdateLocalKeyFrames -> dict of its arguments.  Every map point is observed by the key frames listed in obs."""
    def build(n_kf, frame_obs, cov, child, parent, bad=()):
        # one map point per entry of frame_obs (its observing key frames), all held by the frame
        obs_off, obs_kf = csr(frame_obs)
        kb = np.zeros(n_kf, np.uint8)
        kb[list(bad)] = 1
        co, ck = csr(cov)
        ho, hk = csr(child)
        return {"frame_mp": np.arange(len(frame_obs), dtype=np.int32), "mp_skip": np.zeros(len(frame_obs), np.uint8), "obs_off": obs_off, "obs_kf": obs_kf, "kf_bad": kb, "cov_off": co,
                "cov_kf": ck, "child_off": ho, "child_kf": hk, "parent": np.asarray(parent, np.int32)}
    if name == "parent_break":  # voters 2, 5, 7; 2's parent 0 is new: the expansion ends there and 5 and 7 are never expanded
        n = 10
        cov = [[] for _ in range(n)]; child = [[] for _ in range(n)]
        cov[2] = [5, 3]; cov[5] = [8]; cov[7] = [9]
        child[2] = [4]
        parent = [-1, 0, 0, 2, 2, 1, 1, 1, 5, 7]
        return build(n, [[2, 5], [5, 7], [2]], cov, child, parent)
    if name == "stop_80":  # 79 voters whose parents are voters; each pushes a neighbour of its own: the walk stops once the list holds more than 80
        n = 200
        cov = [[100 + i] if i < 79 else [] for i in range(n)]
        child = [[] for _ in range(n)]
        parent = [-1] + [i - 1 if i < 79 else 0 for i in range(1, n)]
        return build(n, [[i for i in range(79)]], cov, child, parent)
    if name == "tie_max":  # 3 and 6 both receive two votes, 4 one: pKFmax is the first strict maximum, 3
        n = 8
        cov = [[] for _ in range(n)]; child = [[] for _ in range(n)]
        return build(n, [[3, 6], [6, 3], [4]], cov, child, [-1] * n)
    if name == "bad_and_none":  # a bad voter (not pushed, never pKFmax although it has the most votes), a bad neighbour skipped for the next one, a bad child, more than ten neighbours
        n = 20
        cov = [[] for _ in range(n)]; child = [[] for _ in range(n)]
        cov[1] = [2, 9, 10]; cov[4] = [1, 2, 4, 9, 10, 1, 2, 4, 9, 1, 11]  # 4's eleventh neighbour is the only new one: out of reach
        child[1] = [9, 12]
        return build(n, [[1, 2, 4], [2], [2], [4]], cov, child, [-1] * n, bad=(2, 9))
    if name == "no_votes":
        g = build(4, [[]], [[] for _ in range(4)], [[] for _ in range(4)], [-1] * 4)
        return g
    if name == "random":
        rng = np.random.default_rng(11)
        n = 120
        cov = [list(rng.choice(n, rng.integers(0, 15), replace=False)) for _ in range(n)]
        child = [sorted(rng.choice(n, rng.integers(0, 4), replace=False)) for _ in range(n)]
        parent = [-1] + [int(rng.integers(0, i)) for i in range(1, n)]
        g = build(n, [list(rng.choice(40, rng.integers(0, 5), replace=False)) for _ in range(300)], cov, child, parent, bad=tuple(rng.choice(n, 10, replace=False)))
        g["frame_mp"][rng.uniform(size=300) < 0.2] = -1
        g["mp_skip"][rng.uniform(size=300) < 0.1] = 1
        return g
    raise KeyError(name)


GRAPHS = ("parent_break", "stop_80", "tie_max", "bad_and_none", "no_votes", "random")


def chain_map(frames, seed=900, n_kf=20):
    """One synthetic map for the whole chain: the current frame is frame 0 (its key points, an estimated pose), the point table holds a map point per key point twice over
    (local_points), ~20 key frames hold seeded subsets of them, a tenth of the key points carry their map point from the last frame."""
    k, d = frames[0]
    T, pts, blocks, _ = local_points(frames, seed, n=2 * len(k))
    rng = np.random.default_rng(seed + 10)
    n_points = len(pts["skip"])
    lists = []
    for j in range(n_kf):
        l = rng.choice(n_points, 400, replace=False).astype(np.int32)
        l[rng.uniform(size=len(l)) < 0.15] = -1
        lists.append(l)
    kf_off, kf_mp = csr(lists)
    obs = [[] for _ in range(n_points)]
    for j, l in enumerate(lists):
        for mp in l:
            if mp >= 0:
                obs[mp].append(j)
    obs_off, obs_kf = csr(obs)
    cov = [list(rng.choice(n_kf, 6, replace=False)) for _ in range(n_kf)]
    child = [[] for _ in range(n_kf)]
    parent = [-1] + [int(rng.integers(0, j)) for j in range(1, n_kf)]
    for j in range(1, n_kf):
        child[parent[j]].append(j)
    cov_off, cov_kf = csr(cov)
    child_off, child_kf = csr(child)
    kf_bad = np.zeros(n_kf, np.uint8); kf_bad[7] = 1
    frame_mp = np.full(len(k), -1, np.int32)
    have = np.nonzero((rng.uniform(size=len(k)) < 0.1) & (pts["skip"][:len(k)] == 0))[0]
    frame_mp[have] = have  # point i is the landmark of key point i
    n_obs = np.diff(obs_off).astype(np.int32)
    return {"T": T, "pts": pts, "bad": pts["skip"].copy(), "n_obs": n_obs, "kf_off": kf_off, "kf_mp": kf_mp, "obs_off": obs_off, "obs_kf": obs_kf, "kf_bad": kf_bad, "cov_off": cov_off,
            "cov_kf": cov_kf, "child_off": child_off, "child_kf": child_kf, "parent": np.asarray(parent, np.int32), "frame_mp": frame_mp, "n_kf": n_kf}


CHAIN_FRAME_ID = 10


def chain_pose7(cm):
    from cube_slam_amd import synth
    return synth._pose7(np.asarray(cm["T"][0], f64).reshape(3, 3), np.asarray(cm["T"][1], f64))


def track_local_map(oracle, frame, cm, th=1.0):
    """Tracking::TrackLocalMap (Tracking.cc:1356-1416) over chain_map's arrays, monocular, not just relocalised (th = 1): UpdateLocalKeyFrames, UpdateLocalPoints,
    SearchLocalPoints, the oracle's PoseOptimization and the statistics loop.  frame = sim3_restatement.make_frame of the current frame."""
    keys = frame[0]
    pts, bad, n_obs = cm["pts"], cm["bad"], cm["n_obs"]
    frame_mp = cm["frame_mp"].copy()
    has = frame_mp >= 0
    frame_mp[has & (bad[np.where(has, frame_mp, 0)] != 0)] = -1
    local_kf, kfmax = update_local_keyframes(frame_mp, bad, cm["obs_off"], cm["obs_kf"], cm["kf_bad"], cm["cov_off"], cm["cov_kf"], cm["child_off"], cm["child_kf"], cm["parent"])
    off, mp = csr([cm["kf_mp"][cm["kf_off"][j]:cm["kf_off"][j + 1]] for j in local_kf])
    lp = update_local_points(off, mp, bad)
    seen = np.zeros(len(bad), bool)
    seen[frame_mp[frame_mp >= 0]] = True  # mnLastFrameSeen == mCurrentFrame.mnId
    sub = {k: v[lp] for k, v in pts.items()}
    sub["skip"] = (seen[lp] | (bad[lp] != 0)).astype(np.uint8)
    tb = np.zeros(len(keys), np.uint8)
    held = frame_mp >= 0
    tb[held] = n_obs[frame_mp[held]] > 0
    s = search_local_points(oracle, frame, *cm["T"], sub, (n_obs[lp] > 0).astype(np.uint8), INTR, BOUNDS, LOG_SF, SF, th, 0.8, tb)
    got = s["train_match"] >= 0
    frame_mp[got] = lp[s["train_match"][got]]
    idx = np.nonzero(frame_mp >= 0)[0]
    obs = np.stack([keys["x"][idx], keys["y"][idx], np.full(len(idx), -1.0, f32)], axis=1).astype(f64)
    isg = (f32(1.0) / (SF * SF)).astype(f32)
    pose, flags, _ = oracle.pose_optimization(pts["world_pos"][frame_mp[idx]].astype(f64), obs, isg[keys["octave"][idx]].astype(f64), np.asarray(INTR, f32).astype(f64), chain_pose7(cm))
    outlier = np.zeros(len(keys), np.uint8)
    outlier[idx] = flags
    inliers = int(sum(1 for i in idx if not outlier[i] and n_obs[frame_mp[i]] > 0))
    return {"local_kf": local_kf, "kf_max": kfmax, "local_points": lp, "search": s, "frame_mp": frame_mp, "pose": pose, "outlier": outlier, "inliers": inliers, "ok": inliers >= 30}


def chain_objects(frames, cm):
    """The Map and TrackedFrame of cube_slam_amd.tracking for chain_map's arrays."""
    from cube_slam_amd.tracking import Map, TrackedFrame
    k, d = frames[0]
    pts = cm["pts"]
    m = Map(world_pos=pts["world_pos"], normal=pts["normal"], min_distance=pts["min_distance"], max_distance=pts["max_distance"], desc=pts["mp_desc"], bad=cm["bad"], n_obs=cm["n_obs"],
            obs_off=cm["obs_off"], obs_kf=cm["obs_kf"], kf_off=cm["kf_off"], kf_mp=cm["kf_mp"], kf_bad=cm["kf_bad"], cov_off=cm["cov_off"], cov_kf=cm["cov_kf"], child_off=cm["child_off"],
            child_kf=cm["child_kf"], parent=cm["parent"])
    F = TrackedFrame(CHAIN_FRAME_ID, k, d, BOUNDS, cm["frame_mp"], *cm["T"], INTR, LOG_SF, SF, (f32(1.0) / (SF * SF)).astype(f32), chain_pose7(cm))
    return m, F


def pack(arrays):
    """The array file of tests/cpp/tracking_mirror.cpp: per array an int64 byte count and the bytes."""
    out = b""
    for a in arrays:
        a = np.ascontiguousarray(a)
        out += np.int64(a.nbytes).tobytes() + a.tobytes()
    return out


def graph_arrays(g):
    i32, u8 = np.int32, np.uint8
    return [g["frame_mp"].astype(i32), g["mp_skip"].astype(u8), g["obs_off"].astype(i32), g["obs_kf"].astype(i32), g["kf_bad"].astype(u8), g["cov_off"].astype(i32), g["cov_kf"].astype(i32),
            g["child_off"].astype(i32), g["child_kf"].astype(i32), g["parent"].astype(i32)]


def chain_arrays(frames, cm):
    from cube_slam_amd.orb import KEYPOINT_DTYPE
    k, d = frames[0]
    pts = cm["pts"]
    g = {"frame_mp": cm["frame_mp"], "mp_skip": cm["bad"], **{key: cm[key] for key in ("obs_off", "obs_kf", "kf_bad", "cov_off", "cov_kf", "child_off", "child_kf", "parent")}}
    return graph_arrays(g) + [pts["world_pos"].astype(f32), pts["normal"].astype(f32), pts["min_distance"].astype(f32), pts["max_distance"].astype(f32), pts["mp_desc"].astype(np.uint8),
                              cm["n_obs"].astype(np.int32), cm["kf_off"].astype(np.int32), cm["kf_mp"].astype(np.int32), np.ascontiguousarray(k, KEYPOINT_DTYPE), d.astype(np.uint8),
                              np.asarray(BOUNDS, f32), np.asarray(cm["T"][0], f32), np.asarray(cm["T"][1], f32), np.asarray(cm["T"][2], f32), np.asarray(INTR + (LOG_SF,), f32), SF.astype(f32),
                              (f32(1.0) / (SF * SF)).astype(f32), chain_pose7(cm).astype(f64), np.asarray([CHAIN_FRAME_ID], np.int32)]
