"""TEST INFRASTRUCTURE: seeded cases for the local-mapping tests -- scenes of a current key frame and its neighbours with per-neighbour tables of best matches (the stand-in for
ORBmatcher(0.6, false).SearchForTriangulation, tests/local_mapping_restatement.py::table_search), observation sets for ComputeDistinctiveDescriptors and point clouds for
UpdateNormalAndDepth.  tests/test_local_mapping_patterns.py checks on the CPU that each case holds what its name promises."""
import functools

import numpy as np

from tests import local_mapping_restatement as R

F = np.float32
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
MB = 0.08
MBF = MB * FX
N_LEVELS = 8
SF = (F(1.2) ** np.arange(N_LEVELS, dtype=np.float32)).astype(np.float32)
SIGMA2 = (SF * SF).astype(np.float32)


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    M = np.eye(3)
    M[i, i] = c; M[j, j] = c; M[i, j] = -s; M[j, i] = s
    return M


def pose(Rm, centre):
    """(Rcw, tcw, Ow) as float32 for a camera at `centre` with world-to-camera rotation Rm."""
    Rm = np.asarray(Rm, np.float64)
    t = -Rm @ np.asarray(centre, np.float64)
    return Rm.astype(np.float32), t.astype(np.float32), np.asarray(centre, np.float32)


def project(Rcw, tcw, X):
    xc = np.asarray(Rcw, np.float64) @ np.asarray(X, np.float64) + np.asarray(tcw, np.float64)
    return FX * xc[0] / xc[2] + CX, FY * xc[1] / xc[2] + CY, xc[2]


def keys(n):
    k = np.zeros(n, R.KEYPOINT_DTYPE)
    k["size"] = 31.0; k["class_id"] = -1
    return k


def frame(k, xy, ur, depth, P):
    return R.Frame(k, xy, ur, depth, P[0], P[1], P[2], FX, FY, CX, CY, MBF, MB, SF, SIGMA2, 1.2)


def random_scene(seed, N1, counts, mode, frac_wrong=0.12, frac_far=0.08, skip_frac=0.1, share_idx2=True, short_baselines=True, N2=None):
    """A current key frame with N1 key points of world points in front of it and len(counts) neighbours around it; neighbour n's table of best matches names counts[n] of the
    key points of the current frame.  mode: 'mono' (no key point has a right coordinate), 'stereo' (all have), 'mixed'.  A share of the pairs are wrong correspondences (any
    status may follow) or points too far for any parallax."""
    rng = np.random.RandomState(seed)
    P1 = pose(rot(0, rng.uniform(-2, 2)) @ rot(1, rng.uniform(-2, 2)), rng.uniform(-0.05, 0.05, 3))
    u = rng.uniform(20, 620, N1); v = rng.uniform(20, 460, N1); z = rng.uniform(2, 12, N1)
    far = rng.rand(N1) < (0.0 if mode == "stereo" else frac_far)  # (far points are monocular in both frames, below: a stereo key point is triangulated at any parallax, and
    # the distance of the reference's float SVD from the restatement grows with the depth -- tests/test_local_mapping_restatement_pins.py)
    z[far] = rng.uniform(300, 3000, far.sum())
    Xc = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], axis=1)
    X = (Xc - P1[1].astype(np.float64)) @ P1[0].astype(np.float64)  # Rcw.T (Xc - t)

    def stereo_flags(n):
        return {"mono": np.zeros(n, bool), "stereo": np.ones(n, bool), "mixed": rng.rand(n) < 0.5}[mode]

    k1 = keys(N1)
    k1["x"] = u; k1["y"] = v; k1["octave"] = rng.randint(0, 4, N1)
    s1 = stereo_flags(N1) & ~far
    kf = frame(k1, np.stack([u + 0.25, v - 0.25], axis=1), np.where(s1, u - MBF / z, -1.0), np.where(s1, z, -1.0), P1)
    skip1 = rng.rand(N1) < skip_frac
    free = np.nonzero(~skip1)[0]
    neighbours, best2 = [], []
    for n, cnt in enumerate(counts):
        ang = rng.uniform(0, 2 * np.pi)
        b = rng.uniform(0.005, 0.05) if short_baselines and n % 3 == 1 else rng.uniform(0.25, 0.7)  # every third neighbour closer than mb: the stereo branches, or no parallax at all
        P2 = pose(rot(1, rng.uniform(-4, 4)) @ rot(0, rng.uniform(-3, 3)) @ rot(2, rng.uniform(-3, 3)), [b * np.cos(ang), b * np.sin(ang), rng.uniform(-0.1, 0.1)])
        n2 = max(cnt, 1) + 7 if N2 is None else N2
        k2 = keys(n2)
        k2["x"] = rng.uniform(20, 620, n2); k2["y"] = rng.uniform(20, 460, n2); k2["octave"] = rng.randint(0, 4, n2)
        z2 = rng.uniform(2, 12, n2)
        tab = np.full(N1, -1, np.int32)
        assert cnt <= len(free)
        chosen = np.sort(rng.choice(free, cnt, replace=False))
        slots = rng.permutation(n2)[:cnt]
        for i, j in zip(chosen, slots):
            tab[i] = j
            if rng.rand() < frac_wrong:
                continue  # the key point stays where chance put it
            pu, pv, pz = project(P2[0], P2[1], X[i])
            k2["x"][j] = pu + rng.normal(0, 0.5); k2["y"][j] = pv + rng.normal(0, 0.5); z2[j] = pz
            k2["octave"][j] = np.clip(k1["octave"][i] + rng.randint(-1, 2), 0, N_LEVELS - 1)
        if share_idx2 and cnt >= 2:
            tab[chosen[1]] = tab[chosen[0]]  # two key points of the current frame with the same best match: nothing claims a key point of the neighbour
        s2 = stereo_flags(n2)
        s2[tab[chosen[far[chosen]]]] = False
        zz = np.where(z2 > 0.1, z2, 1.0)
        neighbours.append(frame(k2, np.stack([k2["x"] + 0.25, k2["y"] - 0.25], axis=1), np.where(s2, k2["x"] - MBF / zz, -1.0), np.where(s2, zz, -1.0), P2))
        best2.append(tab)
    return {"kf": kf, "neighbours": neighbours, "best2": best2, "skip1": skip1}


COUNTS = (0, 1, 63, 64, 65, 300)


def _cycle(n):
    return [COUNTS[(i * 5 + 2) % 6] for i in range(n)]


SCENES = {}
for _c in COUNTS:
    SCENES["n1_mixed_%d" % _c] = (100 + _c, 400, [_c], "mixed")
SCENES.update({
    "n3_mono_gap": (201, 400, [63, 0, 65], "mono"),       # a neighbour with zero pairs in the middle
    "n3_stereo": (202, 400, [300, 1, 64], "stereo"),
    "n3_mixed": (203, 400, [65, 64, 300], "mixed"),
    "n20_mixed": (204, 400, _cycle(20), "mixed"),
    "n20_mono": (205, 400, _cycle(20)[::-1], "mono"),
})


def claim_0_2():
    """Three neighbours that see all 12 key points; key point 5 is accepted by neighbours 0 and 2 and rejected by 1 (its key point there is 25 px off), key points 3 and 4 have
    the same best match in neighbour 0."""
    s = random_scene(301, 12, [12, 12, 12], "mono", frac_wrong=0.0, frac_far=0.0, skip_frac=0.0, share_idx2=False, short_baselines=False)
    j = s["best2"][1][5]
    s["neighbours"][1].keysUn["y"][j] += F(25.0)
    s["best2"][0][4] = s["best2"][0][3]
    return s


def _setkp(f, i, u, v, octave, depth=None):
    f.keysUn["x"][i] = u; f.keysUn["y"][i] = v; f.keysUn["octave"][i] = octave
    f.keys_xy[i] = (u, v)
    if depth is None:
        f.u_right[i] = -1; f.depth[i] = -1
    else:
        f.u_right[i] = F(u) - F(MBF) / F(depth if depth > 0 else 5.0); f.depth[i] = depth


STATUS_ROWS = {  # (neighbour, idx1) -> the status the row is built for
    (0, 0): R.CREATED, (0, 1): R.PARALLAX, (0, 2): R.Z1, (0, 3): R.REPROJ1, (0, 4): R.REPROJ2, (0, 5): R.SCALE, (0, 6): R.CREATED, (0, 14): R.PARALLAX, (0, 15): R.CREATED,
    (1, 0): R.CLAIMED, (1, 7): R.CREATED, (1, 8): R.CREATED, (1, 9): R.PARALLAX, (1, 10): R.STEREO_NO_DEPTH,
    (2, 11): R.Z2, (3, 12): R.Z1, (4, 13): R.ZERO_DIST,
}
STATUS_BRANCH = {(0, 0): "svd", (0, 6): "svd", (1, 7): "stereo1", (1, 8): "stereo2", (1, 9): None, (1, 10): "stereo1", (2, 11): "stereo1", (3, 12): "stereo2", (4, 13): "stereo1"}


@functools.lru_cache(maxsize=None)
def statuses():
    """One call whose pairs hit every status but w == 0, each of the three x3D branches and the `continue` at :467, with cosParallaxRays on both sides of 0.9998 (rows (0, 14)
    and (0, 15): mono points near the axis at depths 21 and 19, where a baseline of 0.4 subtends 0.02 rad at depth 20).  Neighbour 0 has a baseline of 0.4 along x, neighbour 1 one of 0.01 (shorter than mb: the stereo
    branches), neighbour 2 stands 20 ahead and neighbour 3 20 behind, neighbour 4 is neighbour 1 with the stored Ow set to the x3D of row 13."""
    N1 = 16
    P1 = pose(np.eye(3), [0, 0, 0])
    kf = frame(keys(N1), np.zeros((N1, 2)), np.full(N1, -1.0), np.full(N1, -1.0), P1)
    Ps = [pose(np.eye(3), [0.4, 0, 0]), pose(np.eye(3), [0.01, 0, 0]), pose(np.eye(3), [0, 0, 20.0]), pose(np.eye(3), [0, 0, -20.0]), pose(np.eye(3), [0.01, 0, 0])]
    nb = [frame(keys(N1), np.zeros((N1, 2)), np.full(N1, -1.0), np.full(N1, -1.0), P) for P in Ps]
    best2 = [np.full(N1, -1, np.int32) for _ in Ps]

    def point(i, uv=None, z=5.0):
        u, v = uv if uv else (100.0 + 30 * i, 80.0 + 20 * i)
        return np.array([(u - CX) / FX * z, (v - CY) / FY * z, z]), u, v

    def pair(n, i, z=5.0, oct1=1, oct2=1, st1=False, st2=False, du=0.0, dv=0.0, depth1=None, same_xn=False, uv=None):
        X, u, v = point(i, uv, z)
        _setkp(kf, i, u, v, oct1, (depth1 if depth1 is not None else z) if st1 else None)
        pu, pv, pz = project(Ps[n][0], Ps[n][1], X) if not same_xn else (u, v, z)
        _setkp(nb[n], i, pu + du, pv + dv, oct2, (pz if pz > 0 else z) if st2 else None)
        best2[n][i] = i

    pair(0, 0)                                  # created, mono / mono
    pair(0, 1, z=5000.0)                        # no parallax
    pair(0, 2, du=60.0)                         # negative disparity: the rays meet behind both cameras
    pair(0, 3, oct1=0, oct2=0, dv=8.0)          # 4 px off in both views at level 0
    pair(0, 4, oct1=7, oct2=0, dv=8.0)          # ... which level 7 forgives in the current key frame
    pair(0, 5, oct1=0, oct2=7)                  # same distance, seven levels apart
    pair(0, 6, st1=True)                        # stereo key point with parallax: triangulated
    pair(0, 14, z=21.0, uv=(330.0, 250.0))                      # cosParallaxRays just above 0.9998
    pair(0, 15, z=19.0, uv=(310.0, 230.0))                      # ... and just below
    X0 = point(0)[0]
    pu, pv, _ = project(Ps[1][0], Ps[1][1], X0)
    _setkp(nb[1], 0, pu, pv, 1)
    best2[1][0] = 0                             # claimed by neighbour 0
    pair(1, 7, st1=True)                        # stereo 1 closer than the baseline: UnprojectStereo of the current key frame
    pair(1, 8, st2=True)                        # ... of the neighbour
    pair(1, 9)                                  # neither: continue
    pair(1, 10, st1=True, depth1=-1.0)          # a right coordinate without depth
    pair(2, 11, st1=True, same_xn=True)         # the point lies behind the neighbour that stands ahead
    pair(3, 12, st2=True, same_xn=True)         # the neighbour's point lies behind the current key frame
    pair(4, 13, st1=True)
    x13 = R.triangulate_pair(kf, 13, nb[4], 13)[1]
    nb[4].Ow[:] = x13                           # as stored: the library reads Ow, it does not derive it
    return {"kf": kf, "neighbours": nb, "best2": best2, "skip1": np.zeros(N1, bool)}


def w_zero():
    """The one status no camera reaches: both 'rotations' have a zero first column and both translations are zero, so columns 0 and 3 of A are zero, the first of them wins and
    the vector is (1, 0, 0, 0).  The library reads Rcw as stored."""
    R1 = np.diag([0.0, 1.0, 1.0])
    R2 = R1 @ rot(0, 20)
    z3 = [0, 0, 0]
    kf = frame(keys(1), np.zeros((1, 2)), [-1.0], [-1.0], (R1.astype(np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)))
    n0 = frame(keys(1), np.zeros((1, 2)), [-1.0], [-1.0], (R2.astype(np.float32), np.zeros(3, np.float32), np.array(z3, np.float32)))
    _setkp(kf, 0, 300.0, 200.0, 0); _setkp(n0, 0, 310.0, 260.0, 0)
    return {"kf": kf, "neighbours": [n0], "best2": [np.array([0], np.int32)], "skip1": np.zeros(1, bool)}


def cos_zero():
    """cosParallaxRays on both sides of 0: neighbours turned by 89 and 91 degrees about y, key points at the principal points."""
    kf = frame(keys(1), np.zeros((1, 2)), [-1.0], [-1.0], pose(np.eye(3), [0, 0, 0]))
    _setkp(kf, 0, CX, CY, 0)
    nb = []
    for deg in (89.0, 91.0):
        f = frame(keys(1), np.zeros((1, 2)), [-1.0], [-1.0], pose(rot(1, deg), [3.0, 0, 3.0]))
        _setkp(f, 0, CX, CY, 0)
        nb.append(f)
    return {"kf": kf, "neighbours": nb, "best2": [np.array([0], np.int32)] * 2, "skip1": np.zeros(1, bool)}


SPECIAL = {"claim_0_2": claim_0_2, "statuses": statuses, "w_zero": w_zero, "cos_zero": cos_zero}
ALL = sorted(SCENES) + sorted(SPECIAL)


@functools.lru_cache(maxsize=None)
def scene(name):
    return SPECIAL[name]() if name in SPECIAL else random_scene(*SCENES[name])


@functools.lru_cache(maxsize=None)
def judged(name):
    """The restatement's outputs for a scene, computed once."""
    s = scene(name)
    return R.expected_outputs(s["kf"], s["neighbours"], R.table_search(s["best2"]), s["skip1"])


# ---- ComputeDistinctiveDescriptors
DESC_N = (1, 2, 3, 4, 63, 64, 65, 200)


def descriptor_sets(kind, seed=0):
    """(obs_off, desc): 'sizes' -- one point per N of DESC_N, noisy copies of one descriptor; 'equal' -- all descriptors of a point equal (the first index wins); 'ties' --
    drawn from 3 distinct descriptors; 'mixed' -- 2 000 points of 0..40 observations (and one of 130), among them empty runs."""
    rng = np.random.RandomState(500 + seed)

    def noisy(n, flips):
        base = rng.randint(0, 256, 32).astype(np.uint8)
        d = np.repeat(base[None], n, axis=0)
        for r in range(n):
            bits = rng.choice(256, rng.randint(0, flips + 1), replace=False)
            for b in bits:
                d[r, b >> 3] ^= np.uint8(1 << (b & 7))
        return d

    if kind == "sizes":
        sets = [noisy(n, 60) for n in DESC_N]
    elif kind == "equal":
        sets = [np.repeat(rng.randint(0, 256, (1, 32)).astype(np.uint8), n, axis=0) for n in DESC_N]
    elif kind == "ties":
        sets = []
        for n in DESC_N:
            three = rng.randint(0, 256, (3, 32)).astype(np.uint8)
            sets.append(three[rng.randint(0, 3, n)])
    elif kind == "mixed":
        ns = rng.randint(0, 41, 2000)
        ns[7] = 0; ns[1999] = 0; ns[1000] = 130
        sets = [noisy(int(n), 40) if rng.rand() < 0.7 else rng.randint(0, 256, (3, 32)).astype(np.uint8)[rng.randint(0, 3, int(n))] for n in ns]
    else:
        raise KeyError(kind)
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    desc = np.concatenate([s.reshape(-1, 32) for s in sets]).astype(np.uint8) if off[-1] else np.zeros((0, 32), np.uint8)
    return off, desc


# ---- UpdateNormalAndDepth
NORMAL_N = (1, 64, 65, 5000)


@functools.lru_cache(maxsize=None)
def normal_case(n_points):
    """n_points points with 1..40 observations among 50 key frames; point 0 has its reference key frame last in its run, the last point of a case of more than one has no
    observation."""
    rng = np.random.RandomState(700 + n_points)
    n_kf = 50
    kf_Ow = rng.uniform(-3, 3, (n_kf, 3)).astype(np.float32)
    pos = (rng.uniform(-1, 1, (n_points, 3)) * [4, 4, 1] + [0, 0, 9]).astype(np.float32)
    runs = []
    for p in range(n_points):
        runs.append(rng.choice(n_kf, rng.randint(1, 41), replace=False).astype(np.int32))
    if n_points > 1:
        runs[-1] = np.zeros(0, np.int32)
    if n_points > 2:
        runs[1] = rng.choice(n_kf, 40, replace=False).astype(np.int32)
        runs[2] = runs[2][:1]
    ref_kf = np.array([r[rng.randint(len(r))] if len(r) else 0 for r in runs], np.int32)
    ref_kf[0] = runs[0][-1]
    ref_oct = rng.randint(0, N_LEVELS, n_points).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int32)
    return {"pos": pos, "obs_off": off, "obs_kf": np.concatenate(runs).astype(np.int32), "kf_Ow": kf_Ow, "ref_kf": ref_kf, "ref_octave": ref_oct, "n_kf": n_kf}


@functools.lru_cache(maxsize=None)
def normal_judged(n_points):
    c = normal_case(n_points)
    normal = np.full((n_points, 3), 7.0, np.float32); mind = np.full(n_points, 7.0, np.float32); maxd = np.full(n_points, 7.0, np.float32); upd = np.zeros(n_points, np.uint8)
    return R.update_normal_and_depth_many(c["pos"], c["obs_off"], c["obs_kf"], c["kf_Ow"], c["ref_kf"], c["ref_octave"], SF, normal, mind, maxd, upd)
