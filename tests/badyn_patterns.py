"""Windows for the dynamic-object BA (cs_ba_dyn_*, cube_slam_amd/csrc/badyn.hip) cut from synth.ba_dyn_problem so that they land on the seams of its
device code: pose systems of an exact size NP (blocked Cholesky: one block, a ragged block of two rows, one / two panel workgroups, more than 1024
rows), object vertices relabelled against time (the transposed source of badyn_gather_blocks), gather / Schur / slot lists of exact lengths, a static
point without an active edge, and starts bad enough that Levenberg-Marquardt rejects trials.  Plain numpy; every transform returns a new dict and
leaves its input untouched.  tests/test_badyn_patterns.py (CPU, oracle only) proves that every pattern reaches what it names;
tests/test_zx_badyn_edges_gpu.py runs them on the device."""
import numpy as np

from cube_slam_amd import synth

_OBS = ("obs_cam", "obs_point", "obs_uv", "obs_ur", "obs_inv_sigma2", "obs_level")
_DOBS = ("dobs_cam", "dobs_obj", "dobs_point", "dobs_uv", "dobs_inv_sigma2", "dobs_level")
EST = ("cam_pose", "obj_pose", "vel", "points", "dpoints")


def deviation(a, b):
    """max |a - b| over max |b|: the measure of tests/test_zx_badyn_gpu.py's bars"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)) if a.size else 0.0


# ----------------------------------------------------------------------------------------------- the pose system
def pose_offsets(d):
    """(cam_off, obj_off, vel_off, NP): free cameras in index order, then object vertices, then velocities; 6, 6 and 2 scalars (-1: fixed camera)"""
    fixed = np.asarray(d["cam_fixed"]).astype(int)
    cam_off = np.where(fixed != 0, -1, 6 * (np.cumsum(1 - fixed) - 1))
    n_free, n_o, n_v = int((fixed == 0).sum()), len(d["obj_pose"]), len(d["vel"])
    return cam_off, 6 * n_free + 6 * np.arange(n_o), 6 * (n_free + n_o) + 2 * np.arange(n_v), 6 * (n_free + n_o) + 2 * n_v


def fix_interleaved(d, n_free):
    """The window with exactly n_free free cameras: key frames 0 and 1 stay fixed, the others to fix are spread evenly over the rest of the window
    (fixed cameras between free ones: the pose-system offset of a camera is not six times its index)."""
    n = len(d["cam_pose"])
    extra = n - 2 - n_free
    if extra < 0 or n_free < 0:
        raise ValueError("%d key frames cannot give %d free cameras" % (n, n_free))
    rest = np.arange(2, n)

    def spread(m):  # the middles of m equal bins of the rest
        return rest[((2 * np.arange(m) + 1) * len(rest)) // (2 * m)] if m else rest[:0]
    fixed = np.zeros(n, np.uint8); fixed[:2] = 1
    if extra <= n_free:
        fixed[spread(extra)] = 1
    else:
        fixed[rest] = 1; fixed[spread(n_free)] = 0
    assert int((fixed == 0).sum()) == n_free
    d = dict(d); d["cam_fixed"] = fixed
    return d


def keep_object_vertices(d, keep):
    """The window with only the object vertices of the boolean mask `keep`: the others go with their dynamic observations, motion edges, camera-object
    edges and point-object edges; the cars (velocities, dynamic points) stay."""
    keep = np.asarray(keep, bool)
    new = np.cumsum(keep) - 1
    d2 = dict(d)
    for k in ("obj_pose", "obj_scale", "obj_flags", "obj_key", "obj_true"):
        if k in d:
            d2[k] = np.ascontiguousarray(np.asarray(d[k])[keep])
    d2 = thinned(d2, drop_dobs=np.nonzero(~keep[d["dobs_obj"]])[0])
    d2["dobs_obj"] = new[d2["dobs_obj"]].astype(np.int32)
    m = keep[d["mot_from"]] & keep[d["mot_to"]]
    d2["mot_from"], d2["mot_to"] = new[d["mot_from"][m]].astype(np.int32), new[d["mot_to"][m]].astype(np.int32)
    d2["mot_vel"], d2["mot_dt"] = d["mot_vel"][m], d["mot_dt"][m]
    c = keep[d["cobs_obj"]]
    d2["cobs_cam"], d2["cobs_obj"] = d["cobs_cam"][c], new[d["cobs_obj"][c]].astype(np.int32)
    for k in ("cobs_bbox", "cobs_info", "cobs_level"):
        d2[k] = d[k][c]
    pk = [o for o in range(len(d["pc_obj"])) if keep[d["pc_obj"][o]]]
    off = d["pc_offsets"]
    d2["pc_obj"] = new[d["pc_obj"][pk]].astype(np.int32)
    d2["pc_points"] = np.concatenate([d["pc_points"][off[o]:off[o + 1]] for o in pk]).reshape(-1, 3) if pk else np.zeros((0, 3))
    d2["pc_offsets"] = np.concatenate([[0], np.cumsum([off[o + 1] - off[o] for o in pk])]).astype(np.int32)
    return d2


def sized(NP, seed, n_kf, n_points, n_objects, pts_per_obj, objects_from_kf=0, **kw):
    """A window whose pose system has exactly NP scalars: NP = 6 (free cameras + object vertices) + 2 cars.  The car count fixes NP mod 6, the number
    of fixed cameras the rest; objects_from_kf keeps only the object vertices of the later key frames (the smallest systems)."""
    d = synth.ba_dyn_problem(seed, n_kf=n_kf, n_points=n_points, n_objects=n_objects, pts_per_obj=pts_per_obj, **kw)
    if objects_from_kf:
        d = keep_object_vertices(d, d["obj_key"][:, 1] >= objects_from_kf)
    rest = NP - 2 * len(d["vel"]) - 6 * len(d["obj_pose"])
    if rest % 6 or rest < 0:
        raise ValueError("NP = %d is out of reach with %d cars and %d object vertices" % (NP, len(d["vel"]), len(d["obj_pose"])))
    d = fix_interleaved(d, rest // 6)
    assert pose_offsets(d)[3] == NP
    return d


def chol_launches(NP):
    """(badyn_chol_diag, badyn_chol_panel = badyn_chol_update) launches of one solve: a pivot block per 32 columns, panel and update wherever rows remain"""
    nblk = (NP + 31) // 32
    return nblk, sum(1 for j in range(nblk) if NP - min(32 * (j + 1), NP) > 0)


# ----------------------------------------------------------------------------------------------- relabelling
def reordered(d, seed):
    """The same window with the object vertices relabelled by a seeded permutation (vertex i becomes perm[i], kept as d["obj_perm"]): map order instead
    of time order.  Edge order and every edge's vertex order stay, so motion edges now also run from a higher to a lower pose-system offset.
    Un-permute a result with obj_pose[perm]."""
    n = len(d["obj_pose"])
    perm = np.random.default_rng(seed).permutation(n)
    inv = np.argsort(perm)
    d2 = dict(d)
    for k in ("obj_pose", "obj_scale", "obj_flags", "obj_key", "obj_true"):
        if k in d:
            d2[k] = np.ascontiguousarray(np.asarray(d[k])[inv])
    for k in ("dobs_obj", "mot_from", "mot_to", "cobs_obj", "pc_obj"):
        d2[k] = perm[np.asarray(d[k], int)].astype(np.int32)
    d2["obj_perm"] = perm
    return d2


def free_yaw(d):
    """Every object vertex with whether_fixrollpitch instead of whether_fixrotation (flags 1 | 8): yaw is estimated.  With the rotation fixed the block of
    a motion edge between its two object vertices is -W on the translations, a symmetric matrix, and a transposed source cannot be told from a plain
    one; with yaw free the `from` vertex' yaw moves the predicted position and the block is not symmetric."""
    d2 = dict(d)
    d2["obj_flags"] = np.full(len(d["obj_pose"]), 1 | 8, np.uint8)
    return d2


def motion_weight(d, w):
    """object_velocity_BA_weight = w: the information of the motion edges is ((1, 1, 5) w)^2 (synth uses w = 0.5)"""
    d2 = dict(d)
    d2["mot_info"] = (np.array([1.0, 1.0, 5.0]) * w) ** 2
    return d2


def with_reverse_motion(d, every=3):
    """Every `every`-th motion edge gets a twin that runs the other way over the same two vertices with -dt.  The reference never builds such a pair;
    the list rule allows it, and it is the only way one pose x pose block receives a plain and a transposed source."""
    pick = np.arange(0, len(d["mot_from"]), every)
    d2 = dict(d)
    d2["mot_from"] = np.concatenate([d["mot_from"], np.asarray(d["mot_to"])[pick]]).astype(np.int32)
    d2["mot_to"] = np.concatenate([d["mot_to"], np.asarray(d["mot_from"])[pick]]).astype(np.int32)
    d2["mot_vel"] = np.concatenate([d["mot_vel"], np.asarray(d["mot_vel"])[pick]]).astype(np.int32)
    d2["mot_dt"] = np.concatenate([d["mot_dt"], -np.asarray(d["mot_dt"])[pick]])
    return d2


# ----------------------------------------------------------------------------------------------- the lists, from the rule
def _edges(d):
    """every linearised edge in the device's order (static observations, dynamic observations, motion, camera-object, point-object, local point) as a
    list of vertices (pose-system offset or -1, dimension, landmark or -1)"""
    cam_off, obj_off, vel_off, _ = pose_offsets(d)
    fp = bool(d["fix_points"])
    n_pts = len(d["points"])

    def lvl(name, o):
        return d.get(name) is not None and len(d[name]) and d[name][o] != 0
    out = []
    for o in range(len(d["obs_cam"])):
        c = cam_off[d["obs_cam"][o]]
        if lvl("obs_level", o) or (c < 0 and fp):
            continue
        out.append([(c, 6, -1), (-1, 3, -1 if fp else int(d["obs_point"][o]))])
    for o in range(len(d["dobs_cam"])):
        if not lvl("dobs_level", o):
            out.append([(cam_off[d["dobs_cam"][o]], 6, -1), (obj_off[d["dobs_obj"][o]], 6, -1), (-1, 3, -1 if fp else n_pts + int(d["dobs_point"][o]))])
    for o in range(len(d["mot_from"])):
        out.append([(obj_off[d["mot_from"][o]], 6, -1), (obj_off[d["mot_to"][o]], 6, -1), (vel_off[d["mot_vel"][o]], 2, -1)])
    for o in range(len(d["cobs_cam"])):
        if not lvl("cobs_level", o):
            out.append([(cam_off[d["cobs_cam"][o]], 6, -1), (obj_off[d["cobs_obj"][o]], 6, -1)])
    for o in range(len(d["pc_obj"])):
        out.append([(obj_off[d["pc_obj"][o]], 6, -1)])
    if not fp:
        for i in range(len(d["dpoints"])):
            out.append([(-1, 3, n_pts + i)])
    return out


def list_lengths(d):
    """What cs_ba_dyn_create lists for this window, restated from the rule (not from the library's code):
    * an edge adds one source to the pose x pose block of every pair (i <= j) of its pose vertices that are in the system; the block is keyed by
      (lower offset, higher offset) and the source is transposed when vertex i has the higher offset;
    * every pose vertex in the system with at least one edge owns a gradient target (n_pg of them);
    * a level-0 observation owns a slot per pose vertex in the system (static: its camera; dynamic: its camera and its object vertex), on its point;
      a Schur target block (u >= t) receives every ordered pair of slots of one point whose offsets are (u, t); a pose vertex' slot count is the
      number of slots on it;
    * L counts all points unless they are fixed, n_edges every edge row including the dynamic points' local-point edges and edges off level 0.
    -> {"pb": {(lo, hi): (sources, (rows, columns), plain, transposed)}, "n_pg", "schur": {(u, t): pairs}, "slots": {offset: n}, "L", "n_edges"}"""
    pb, pg = {}, set()
    for verts in _edges(d):
        for i, (oi, di, li) in enumerate(verts):
            if li < 0 and oi >= 0:
                pg.add(int(oi))
            for (oj, dj, _) in verts[i:]:
                if oi < 0 or oj < 0:
                    continue
                key, dim, tr = ((int(oi), int(oj)), (di, dj), 0) if oi <= oj else ((int(oj), int(oi)), (dj, di), 1)
                n, dm, plain, trans = pb.get(key, (0, dim, 0, 0))
                assert dm == dim
                pb[key] = (n + 1, dim, plain + 1 - tr, trans + tr)
    fp = bool(d["fix_points"])
    schur, slots = {}, {}
    if not fp:
        cam_off, obj_off, _, _ = pose_offsets(d)
        per_lm = {}
        lv = d.get("obs_level")
        for o in range(len(d["obs_cam"])):
            if lv is None or not lv[o]:
                per_lm.setdefault(int(d["obs_point"][o]), []).append(int(cam_off[d["obs_cam"][o]]))
        lv = d.get("dobs_level")
        for o in range(len(d["dobs_cam"])):
            if lv is None or not lv[o]:
                per_lm.setdefault(len(d["points"]) + int(d["dobs_point"][o]), []).extend([int(cam_off[d["dobs_cam"][o]]), int(obj_off[d["dobs_obj"][o]])])
        for offs in per_lm.values():
            offs = [x for x in offs if x >= 0]
            for u in offs:
                slots[u] = slots.get(u, 0) + 1
                for t in offs:
                    if u >= t:
                        schur[(u, t)] = schur.get((u, t), 0) + 1
    n_edges = len(d["obs_cam"]) + len(d["dobs_cam"]) + len(d["mot_from"]) + len(d["cobs_cam"]) + len(d["pc_obj"]) + len(d["dpoints"])
    return {"pb": pb, "n_pg": len(pg), "schur": schur, "slots": slots, "L": 0 if fp else len(d["points"]) + len(d["dpoints"]), "n_edges": n_edges}


# ----------------------------------------------------------------------------------------------- thinning
def thinned(d, drop_obs=(), drop_dobs=()):
    """The window without the given rows of obs_* / dobs_*"""
    d2 = dict(d)
    for keys, drop in ((_OBS, drop_obs), (_DOBS, drop_dobs)):
        keep = np.ones(len(d[keys[0]]), bool); keep[np.asarray(drop, int)] = False
        for k in keys:
            if d.get(k) is not None:
                d2[k] = np.ascontiguousarray(np.asarray(d[k])[keep])
    return d2


def dobs_per_vertex(d, counts):
    """Thins dobs_* so that the object vertices with the most dynamic observations, among those seen from a free camera, keep exactly counts[0],
    counts[1], ... of them (the first ones).  With n observations left, the vertex' block with its camera has n + 1 sources (the camera-object edge is
    the last), its Schur block with its camera n pairs and the vertex n slots.  -> (window, the vertices chosen)"""
    cam_off = pose_offsets(d)[0]
    have = np.bincount(d["dobs_obj"], minlength=len(d["obj_pose"]))
    cam_of = {int(o): int(c) for c, o in zip(d["cobs_cam"], d["cobs_obj"])}
    todo, drop, chosen = sorted(counts, reverse=True), [], []
    for oi in np.argsort(-have, kind="stable"):
        if not todo:
            break
        if int(oi) in cam_of and cam_off[cam_of[int(oi)]] >= 0 and have[oi] >= todo[0]:
            rows = np.nonzero(d["dobs_obj"] == oi)[0]
            drop.extend(rows[todo[0]:]); chosen.append((int(oi), todo.pop(0)))
    if todo:
        raise ValueError("no object vertex left with %d dynamic observations" % todo[0])
    return thinned(d, drop_dobs=drop), chosen


def edges_cut_to(d, n_edges):
    """Drops evenly spaced static observations until the window has exactly n_edges edges"""
    ll = list_lengths(d)
    extra = ll["n_edges"] - n_edges
    n = len(d["obs_cam"])
    if extra < 0 or extra > n // 2:
        raise ValueError("cannot cut %d edges to %d with %d static observations" % (ll["n_edges"], n_edges, n))
    return thinned(d, drop_obs=(np.arange(extra) * n) // max(extra, 1)) if extra else dict(d)


def without_active_edge(d, point):
    """Second-stage layout: every observation of static point `point` at level 1.  The point keeps its rows and has no active edge: g2o does not make it
    an active vertex, the device gives it an empty gather list, D = lambda I and a zero step.  It must come back unchanged."""
    d2 = dict(d)
    lvl = np.array(d["obs_level"], np.uint8)
    lvl[np.asarray(d["obs_point"]) == point] = 1
    d2["obs_level"] = lvl
    d2["dead_point"] = int(point)
    return d2


# ----------------------------------------------------------------------------------------------- starts that make LM reject
def _base(seed):
    return dict(synth.ba_dyn_problem(seed, n_kf=8, n_points=120, n_objects=2, pts_per_obj=12))


def _rot_of_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def shaken_centres(seed, sigma=1.0):
    """camera centres of key frames 2.. moved by N(0, sigma) metres (t is that of Tcw: c = -R^T t)"""
    d = _base(seed)
    rng = np.random.default_rng(1000 + seed)
    cam = d["cam_pose"].copy()
    for i in range(2, len(cam)):
        cam[i, :3] -= _rot_of_quat(cam[i, 3:]) @ rng.normal(0, sigma, 3)
    d["cam_pose"] = cam
    return d


def shaken_dpoints(seed, sigma=2.0):
    """dynamic points moved by N(0, sigma) metres in their car's frame: far outside the box, where UnaryLocalPoint is clipped and flat"""
    d = _base(seed)
    d["dpoints"] = d["dpoints"] + np.random.default_rng(2000 + seed).normal(0, sigma, d["dpoints"].shape)
    return d


def shaken_quaternions(seed, sigma=0.15):
    """camera quaternions of key frames 2.. perturbed by N(0, sigma) per component and normalised"""
    d = _base(seed)
    cam = d["cam_pose"].copy()
    cam[2:, 3:] += np.random.default_rng(3000 + seed).normal(0, sigma, cam[2:, 3:].shape)
    cam[:, 3:] /= np.linalg.norm(cam[:, 3:], axis=1, keepdims=True)
    d["cam_pose"] = cam
    return d


def gross_outliers(seed, px=300.0):
    """every third static observation moved by `px` pixels with the Huber widths out of reach: a plain least-squares fit of wrong data"""
    d = _base(seed)
    uv = d["obs_uv"].copy(); uv[::3] += px
    d["obs_uv"] = uv
    for k in ("huber_mono", "huber_stereo", "huber_dyn", "huber_obj"):
        d[k] = 1e9
    return d


# ----------------------------------------------------------------------------------------------- the named set
LADDER = {  # NP -> sized() arguments
    32: dict(seed=39, n_kf=6, n_points=50, n_objects=1, pts_per_obj=10, objects_from_kf=3),    # 2 free cameras + 3 vertices, 1 car
    34: dict(seed=39, n_kf=6, n_points=50, n_objects=2, pts_per_obj=10, objects_from_kf=4),    # 1 + 4, 2 cars
    64: dict(seed=39, n_kf=8, n_points=60, n_objects=2, pts_per_obj=10, objects_from_kf=5),    # 4 + 6, 2 cars
    160: dict(seed=5, n_kf=12, n_points=120, n_objects=2, pts_per_obj=10, objects_from_kf=3),  # 8 + 18, 2 cars
    162: dict(seed=5, n_kf=12, n_points=120, n_objects=3, pts_per_obj=10, objects_from_kf=6),  # 8 + 18, 3 cars
    # badyn_chol_tri runs 1024 threads: its load / store loops take a second pass above 1024 rows, the forward row loop behind the first block
    # (rows 32 + tid) and the backward column loop under the last block (columns < 1088) above 1056.  18 and 2 rows in the last block.
    1042: dict(seed=12, n_kf=116, n_points=200, n_objects=2, pts_per_obj=8),                   # 98 + 75, 2 cars
    1090: dict(seed=12, n_kf=116, n_points=200, n_objects=2, pts_per_obj=8),                   # 106 + 75, 2 cars
}
VERTEX_COUNTS = (6, 7, 8, 10, 11, 15, 16)  # dynamic observations left on seven object vertices: sources 7, 8, 9, 11, 12, 16, 17; pairs / slots as given


def _lists(n_points, n_pg, n_kf, from_kf, seed=24):
    """L = n_points + 48 points, n_pg pose vertices with a gradient, seven object vertices thinned to VERTEX_COUNTS"""
    d = synth.ba_dyn_problem(seed, n_kf=n_kf, n_points=n_points, n_objects=2, pts_per_obj=24)
    d = keep_object_vertices(d, d["obj_key"][:, 1] >= from_kf)
    d = fix_interleaved(d, n_pg - len(d["obj_pose"]) - len(d["vel"]))
    return dobs_per_vertex(d, VERTEX_COUNTS)[0]


def _edges_exact(n_edges, n_pg, seed=24):
    d = synth.ba_dyn_problem(seed, n_kf=6, n_points=70, n_objects=1, pts_per_obj=12)
    return edges_cut_to(fix_interleaved(d, n_pg - len(d["obj_pose"]) - len(d["vel"])), n_edges)


def _dead_point(d):
    """the static point with the most observations loses them all to level 1"""
    return without_active_edge(d, int(np.argmax(np.bincount(d["obs_point"], minlength=len(d["points"])))))


# rejected-trial windows: (builder, seed, iterations); chosen with the oracle so that trials are rejected (several in a row) and the accept / reject
# decisions survive a relabelling of the object vertices (tests/test_badyn_patterns.py re-derives both).  No shaken_dpoints start among seeds 30 to 199
# kept trace, estimates and lambda_final within a tenth of the device bars under relabelling; the builder stays for the next search.
REJECTED = {"rejected_centres": (shaken_centres, 139, 8), "rejected_quaternions": (shaken_quaternions, 191, 8), "rejected_outliers": (gross_outliers, 96, 8)}
_BUILDERS = {
    "lists_L64_pg21": lambda: _lists(16, 21, 10, 3),
    "lists_L65_pg20_mixed": lambda: with_reverse_motion(reordered(motion_weight(free_yaw(_lists(17, 20, 11, 5, seed=36)), 5.0), 5)),
    "edges256_pg10": lambda: _edges_exact(256, 10),
    "edges257_pg11_dead_point": lambda: _dead_point(_edges_exact(257, 11)),
    "edges_le64": lambda: dict(synth.ba_dyn_problem(31, n_kf=4, n_points=8, n_objects=1, pts_per_obj=5)),
    "reordered_np136": lambda: reordered(synth.ba_dyn_problem(41, n_kf=8, n_points=200, n_objects=2, pts_per_obj=16), 1),
    "reordered_np160_yaw": lambda: reordered(motion_weight(free_yaw(sized(160, **LADDER[160])), 5.0), 2),
}
for _np, _kw in LADDER.items():
    _BUILDERS["np%d" % _np] = (lambda n=_np, kw=_kw: sized(n, **kw))
for _name, (_f, _seed, _) in REJECTED.items():
    _BUILDERS[_name] = (lambda f=_f, s=_seed: f(s))
LIST_SEAMS = ("lists_L64_pg21", "lists_L65_pg20_mixed", "edges256_pg10", "edges257_pg11_dead_point", "edges_le64")
REORDERED = ("reordered_np136", "reordered_np160_yaw")
_cache = {}


def build(name):
    """The window `name` (built once; treat it as read-only)"""
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


_ref = {}


def oracle_optimize(oracle, name, iterations):
    """oracle.badyn_optimize on build(name), computed once per (window, iteration count) and shared by the tests (read-only)"""
    if (name, iterations) not in _ref:
        _ref[(name, iterations)] = oracle.badyn_optimize(build(name), iterations)
    return _ref[(name, iterations)]


def order_noise(oracle, name, iterations, perm_seeds=(1, 2)):
    """How far the oracle moves against itself when the object vertices of build(name) are relabelled (a pure reordering of its sums):
    -> (same iterations and lm_trials on every relabelling, largest deviation of the chi2 trace, of any estimate, of lambda_final)"""
    res, st = oracle_optimize(oracle, name, iterations)
    same, d_tr, d_est, d_lam = True, 0.0, 0.0, 0.0
    for s in perm_seeds:
        d2 = reordered(build(name), s)
        r2, s2 = oracle.badyn_optimize(d2, iterations)
        r2["obj_pose"] = r2["obj_pose"][d2["obj_perm"]]
        same = same and s2["iterations"] == st["iterations"] and s2["lm_trials"] == st["lm_trials"]
        if same:
            d_tr = max(d_tr, deviation(s2["chi2_trace"], st["chi2_trace"]))
            d_est = max(d_est, max(deviation(r2[k], res[k]) for k in EST))
            d_lam = max(d_lam, abs(s2["lambda_final"] / st["lambda_final"] - 1))
    return same, d_tr, d_est, d_lam
