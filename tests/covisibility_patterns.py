"""Designed inputs for cs_covisibility_update, cs_keyframe_culling and cs_mappoint_culling (include/cubeslam_hip/covisibility.h): each case is built so that the property in its
name holds, and tests/test_covisibility_patterns.py asserts on the CPU that it does.  Every case is a dict of plain arrays; expected() gives the restatement's answer in the
layout of the C-ABI, computed once per case and shared by the tests."""
import functools

import numpy as np

from cube_slam_amd.covisibility import COUNTER_TILE
from tests import covisibility_restatement as R

TILE = COUNTER_TILE
BAD, DYNAMIC = 1, 2


def table(n_kf, points):
    """points: one dict per point: obs = [(kf, octave, stereo)] (any order; stored ascending), nobs (default: the reference's count, 2 per stereo entry), flags."""
    off, kf, octave, stereo, nobs, flags = [0], [], [], [], [], []
    for p in points:
        obs = sorted(p["obs"])
        kf += [o[0] for o in obs]; octave += [o[1] for o in obs]; stereo += [o[2] for o in obs]
        off.append(len(kf))
        nobs.append(p.get("nobs", sum(2 if o[2] else 1 for o in obs)))
        flags.append(p.get("flags", 0))
    return dict(n_kf=n_kf, n_points=len(points), obs_off=np.array(off, np.int32), obs_kf=np.array(kf, np.int32), obs_octave=np.array(octave, np.int32),
                obs_stereo=np.array(stereo, np.uint8), mp_nobs=np.array(nobs, np.int32), mp_flags=np.array(flags, np.uint8))


def seen_by(kfs, octave=0, **kw):
    return dict(obs=[(k, octave, 0) for k in kfs], **kw)


def lists(slot_lists):
    off = np.concatenate([[0], np.cumsum([len(s) for s in slot_lists])]).astype(np.int32)
    return off, np.array([v for s in slot_lists for v in s], np.int32)


def vote_case(n_kf, points, queries, slot_lists, skip_dynamic=(1,), th=15):
    off, mp = lists(slot_lists)
    return dict(kind="vote", t=table(n_kf, points), query_kf=np.array(queries, np.int32), kf_off=off, kf_mp=mp, skip_dynamic=tuple(skip_dynamic), th=th)


# ---- the vote ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def vote_threshold():
    """Key frame 0 holds 16 points; key frames 1, 2, 3 see 14, 15 and 16 of them."""
    pts = [seen_by([0] + [k for k, n in ((1, 14), (2, 15), (3, 16)) if j < n]) for j in range(16)]
    return vote_case(4, pts, [0], [list(range(16))])


def vote_fallback_tie():
    """Nothing reaches 15; key frames 2 and 4 both have the largest count, 3, key frame 1 has 2."""
    pts = [seen_by([0, 2, 4, 1]), seen_by([0, 2, 4, 1]), seen_by([0, 2, 4])]
    return vote_case(5, pts, [0], [[0, 1, 2]])


def vote_sort_ties():
    """Key frames 1, 3, 5 with weight 16 each and key frame 2 with 17."""
    pts = [seen_by([0, 2] + ([1, 3, 5] if j < 16 else [])) for j in range(17)]
    return vote_case(6, pts, [0], [list(range(17))])


def vote_self_and_skips():
    """The query's own observation; a bad point; a dynamic point, counted or not by the flag; an empty slot; a point only the query sees."""
    pts = [seen_by([0, 1]), seen_by([0, 1, 2], flags=BAD), seen_by([0, 2], flags=DYNAMIC), seen_by([0])]
    return vote_case(3, pts, [0], [[0, 1, 2, -1, 3]], skip_dynamic=(1, 0))


def vote_double_slot():
    """One point in two slots votes twice."""
    return vote_case(2, [seen_by([0, 1])], [0], [[0, -1, 0]])


def vote_empty():
    """Queries whose counter stays empty (no slots; only empty slots and points nobody else sees) around one that has a counter."""
    pts = [seen_by([0]), seen_by([1, 2])]
    return vote_case(4, pts, [3, 0, 1, 0], [[], [-1, 0, -1], [1], [0]])


SEAM_VOTERS = (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 3 * TILE + 4)


def vote_tile_seam():
    """n_kf = 3 TILE + 5 with voters on both sides of every seam of the counter tile, voter i with weight i + 1; queried from key frame 0 and from the voter at TILE (whose own
    index is then not counted)."""
    n = len(SEAM_VOTERS)
    pts = [seen_by([0] + [v for i, v in enumerate(SEAM_VOTERS) if j <= i]) for j in range(n)]
    return vote_case(3 * TILE + 5, pts, [0, TILE], [list(range(n)), list(range(n))], th=3)


# ---- key-frame culling -------------------------------------------------------------------------------------------------------------------------------------------------------
def cull_case(n_kf, points, local_kf, slot_lists, octaves=None, depths=None, th_depth=None, monocular=1, kf_flags=None, th_obs=3):
    """slot_lists[i]: the points of local_kf[i]; octaves / depths per slot default to 0 / 1."""
    off, mp = lists(slot_lists)
    flat = lambda v, d, dt: np.full(len(mp), d, dt) if v is None else np.array([x for s in v for x in s], dt)
    n = len(local_kf)
    return dict(kind="cull", t=table(n_kf, points), local_kf=np.array(local_kf, np.int32), kf_off=off, kf_mp=mp, slot_octave=flat(octaves, 0, np.int32),
                slot_depth=flat(depths, 1.0, np.float32), kf_th_depth=np.full(n, 40.0, np.float32) if th_depth is None else np.array(th_depth, np.float32), monocular=monocular,
                kf_flags=np.zeros(n, np.uint8) if kf_flags is None else np.array(kf_flags, np.uint8), th_obs=th_obs)


def cull_boundary():
    """Four key frames with points of their own (the other observers, 10 .. 12, are not in the list): nMPs 10 with nRedundant 9 (kept) and 10 (culled), nMPs 20 with 18 (kept)
    and 19 (culled)."""
    pts, slots = [], []
    for kf, (n, red) in enumerate(((10, 9), (10, 10), (20, 18), (20, 19))):
        slots.append(list(range(len(pts), len(pts) + n)))
        pts += [seen_by([kf, 10, 11, 12]) if j < red else seen_by([kf, 10, 11]) for j in range(n)]
    return cull_case(13, pts, [0, 1, 2, 3], slots)


def cull_level_seam():
    """One key frame, slots at octave 2.  a: others at octave 3 count (slot + 1); b: one of three at 4 does not; c: four entries but nObs == th_obs; d: the same entries with a
    stereo one, nObs 5; e: nObs 5 from two stereo observers, but only two entries of others."""
    pts = [dict(obs=[(0, 2, 0), (1, 3, 0), (2, 3, 0), (3, 3, 0)]), dict(obs=[(0, 2, 0), (1, 4, 0), (2, 3, 0), (3, 3, 0)]),
           dict(obs=[(0, 2, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)], nobs=3), dict(obs=[(0, 2, 1), (1, 0, 0), (2, 0, 0), (3, 0, 0)]), dict(obs=[(0, 2, 0), (1, 0, 1), (2, 0, 1)])]
    return cull_case(4, pts, [0], [[0, 1, 2, 3, 4]], octaves=[[2] * 5])


def cull_depth_and_dynamic():
    """A stereo key frame: depth above mThDepth, below 0, exactly mThDepth (counts), a dynamic point, a bad point, an empty slot, and two plain redundant points."""
    pts = [seen_by([0, 1, 2, 3]) for _ in range(3)] + [seen_by([0, 1, 2, 3], flags=DYNAMIC), seen_by([0, 1, 2, 3], flags=BAD)] + [seen_by([0, 1, 2, 3]) for _ in range(2)]
    return cull_case(4, pts, [0], [[0, 1, 2, 3, 4, -1, 5, 6]], depths=[[40.5, -1.0, 40.0, 1.0, 1.0, 1.0, 1.0, 1.0]], th_depth=[40.0], monocular=0)


def _unmakes(kf_flags=None):
    p1 = [seen_by([0, 2, 3, 4, 5]) for _ in range(10)]
    p2 = [seen_by([0, 1, 2, 3]) for _ in range(10)]
    return cull_case(6, p1 + p2, [0, 1], [list(range(20)), list(range(10, 20))], kf_flags=kf_flags)


def cull_erase_unmakes():
    """A = 0 holds 10 points seen by A and four others and 10 seen by A, B = 1 and two others; B holds only the latter.  On the initial state both are redundant; in sequence A
    goes, B's points fall to nObs 3 and B stays."""
    return _unmakes()


def cull_erase_makes():
    """B = 1 holds 9 redundant points and one point seen by {A, B, X} with nObs 3: 9 of 10, kept on the initial state.  A = 0 goes first (10 of 11), that point turns bad, and
    B is 9 of 9."""
    pts = [seen_by([0, 3, 4, 5]) for _ in range(10)] + [seen_by([0, 1, 2])] + [seen_by([1, 3, 4, 5]) for _ in range(9)]
    return cull_case(6, pts, [0, 1], [list(range(11)), list(range(10, 20))])


def cull_not_erase():
    """cull_erase_unmakes with mbNotErase on A: verdict 2, nothing changes, and B is judged on the initial state (culled)."""
    return _unmakes(kf_flags=[2, 0])


def cull_stereo_decrement():
    """A = 0 goes.  Its own entry is stereo on points 0..3 (nObs 5 -> 3, alive) and on 4..6 (nObs held at 4 -> 2, bad), mono on 7..9 (4 -> 3).  Point 0 sits in two slots: the
    second is a no-op (twice would leave 1 and turn it bad)."""
    others = [(3, 0, 0), (4, 0, 0), (5, 0, 0)]
    pts = [dict(obs=[(0, 0, 1)] + others) for _ in range(4)] + [dict(obs=[(0, 0, 1)] + others, nobs=4) for _ in range(3)] + [dict(obs=[(0, 0, 0)] + others) for _ in range(3)]
    return cull_case(6, pts, [0], [list(range(10)) + [0]])


def cull_id0():
    """The first key frame of the list has mnId == 0 and would be redundant: skipped, nothing changes; the second is judged on the initial state."""
    return _unmakes(kf_flags=[1, 0])


# ---- map-point culling -------------------------------------------------------------------------------------------------------------------------------------------------------
MPCULL_ROWS = (  # flags, found, visible, first_kf_id, nobs -> case (current_kf_id = 10, th_obs = 3)
    (0, 4, 4, 9, 1, 0), (BAD, 4, 4, 9, 5, 1), (DYNAMIC, 4, 4, 9, 5, 1), (0, 1, 5, 9, 5, 2), (0, 4, 4, 8, 3, 3), (0, 4, 4, 7, 4, 4),
    (0, 1, 4, 9, 5, 0),   # a ratio of exactly 0.25 is not below it
    (0, 0, 0, 9, 5, 0),   # 0 / 0 = NaN: not case 2
    (0, 1, 0, 9, 5, 0),   # 1 / 0 = inf: not case 2
    (0, 0, 0, 7, 5, 4),   # ... and the later cases still apply
    (BAD, 0, 9, 7, 1, 1),  # precedence: 1 before 2
    (0, 0, 9, 7, 1, 2),   # 2 before 3
    (0, 4, 4, 7, 3, 3),   # 3 before 4
    (0, 4, 4, 8, 4, 0),   # two key frames old with enough observations stays
    (0, 4, 4, 12, 1, 0),  # a first key frame behind the current one: the difference is negative
)


def mpcull_cases():
    rows = np.array(MPCULL_ROWS, np.int64)
    pts = [dict(obs=[], nobs=int(r[4]), flags=int(r[0])) for r in rows]
    recent = list(range(len(rows))) + [4, 0]  # (a point may stand in the list twice: entries are independent)
    return dict(kind="mpcull", t=table(1, pts), recent=np.array(recent, np.int32), mp_found=rows[:, 1].astype(np.int32), mp_visible=rows[:, 2].astype(np.int32),
                mp_first_kf_id=rows[:, 3].astype(np.int32), current_kf_id=10, th_obs=3, want=np.array([int(rows[i][5]) for i in recent], np.uint8))


# ---- seeded random maps ------------------------------------------------------------------------------------------------------------------------------------------------------
RANDOM_SIZES = {0: (40, 2000, 12), 1: (17, 300, 5), 2: (5, 40, 3)}  # seed: key frames, points, observations per point at most


def random_map(seed):
    """A map with every kind of entry: bad and dynamic points, stereo observations, nObs off the entry count, empty slots, double slots, slots whose point does not observe the
    key frame.  Returns the table, the slot lists of every key frame with octaves and depths, and the point-side arrays of MapPointCulling."""
    n_kf, n_points, max_obs = RANDOM_SIZES[seed]
    rng = np.random.default_rng(1000 + seed)
    pts, holders = [], [[] for _ in range(n_kf)]
    for p in range(n_points):
        most = min(max_obs, n_kf)
        kfs = rng.choice(n_kf, size=int(rng.integers(most - 1, most + 1) if rng.random() < 0.9 else rng.integers(1, most + 1)), replace=False)
        base = int(rng.integers(1, 6))  # the levels of one point lie close together, so that most of its observations count for each other
        obs = [(int(k), base + int(rng.choice([-1, 0, 0, 0, 0, 0, 0, 1, 2, 3], p=[.05, .15, .15, .15, .15, .1, .1, .1, .03, .02])), int(rng.random() < 0.3)) for k in kfs]
        d = dict(obs=obs, flags=int(rng.choice([0, 0, 0, 0, 0, 0, 0, 0, BAD, DYNAMIC])))
        if rng.random() < 0.1:
            d["nobs"] = len(obs)  # counted one per entry, as under use_dynamic_klt_features
        pts.append(d)
        for k, octave, _ in obs:
            holders[k].append((p, octave))
    slots, octaves, depths = [], [], []
    for k in range(n_kf):
        h = list(holders[k])
        extra = int(rng.integers(0, 4))
        h += [(-1, 0)] * extra + [h[int(rng.integers(0, len(h)))] for _ in range(extra if h else 0)] + [(int(rng.integers(0, n_points)), 3) for _ in range(extra)]
        order = rng.permutation(len(h))
        slots.append([h[i][0] for i in order]); octaves.append([h[i][1] for i in order])
        depths.append([float(v) for v in rng.choice([1.0, 5.0, 39.0, 41.0, -1.0], size=len(h), p=[0.5, 0.3, 0.15, 0.03, 0.02])])
    return dict(n_kf=n_kf, points=pts, slots=slots, octaves=octaves, depths=depths, found=rng.integers(0, 9, n_points).astype(np.int32),
                visible=rng.integers(0, 12, n_points).astype(np.int32), first=rng.integers(0, 8, n_points).astype(np.int32))


def random_vote(seed):
    m = random_map(seed)
    queries = list(range(m["n_kf"]))
    return vote_case(m["n_kf"], m["points"], queries, m["slots"], skip_dynamic=(1, 0), th=(15, 4, 2)[seed])


def random_cull(seed):
    m = random_map(seed)
    rng = np.random.default_rng(2000 + seed)
    local = [int(k) for k in rng.permutation(m["n_kf"])[:max(2, (3 * m["n_kf"]) // 4)]]
    flags = [int(v) for v in rng.choice([0, 0, 0, 0, 1, 2], size=len(local))]
    flags[1], flags[-1] = 2, 1  # mbNotErase early in the list, where the key frames are still redundant
    pick = lambda v: [v[k] for k in local]
    return cull_case(m["n_kf"], m["points"], local, pick(m["slots"]), octaves=pick(m["octaves"]), depths=pick(m["depths"]), th_depth=[40.0] * len(local), monocular=seed == 1,
                     kf_flags=flags, th_obs=(3, 3, 2)[seed])


def random_mpcull(seed):
    m = random_map(seed)
    rng = np.random.default_rng(3000 + seed)
    t = table(m["n_kf"], m["points"])
    recent = rng.integers(0, t["n_points"], size=min(300, t["n_points"])).astype(np.int32)
    return dict(kind="mpcull", t=t, recent=recent, mp_found=m["found"], mp_visible=m["visible"], mp_first_kf_id=m["first"], current_kf_id=6, th_obs=(3, 2, 1)[seed])


# ---- the seams of the workgroup-wide scans (block_excl_scan of csrc/common.h) under the three kernels that call them, over tests/compaction_seams.py ------------------------
PER_THREAD = TILE // 256  # covis_vote: the consecutive counters of one thread


def seam_vote_counters(n, fl):
    """covis_vote: the counters of thread i (key frames PER_THREAD i ...) hold a voter where fl[i] is set, at a place in the thread's stretch that moves with i; every
    third voter has weight 2 (th = 2: some reach it, some do not).  The query is the last key frame."""
    voters = [PER_THREAD * int(i) + int(i) % PER_THREAD for i in np.flatnonzero(fl)]
    q = PER_THREAD * n
    return vote_case(q + 1, [seen_by([q] + voters), seen_by([q] + voters[::3])], [q], [[0, 1]], th=2)


def seam_vote_queries(n, fl):
    """covis_offsets: n queries; the flagged ones have a counter of three key frames, one of them at the threshold, the others none."""
    pts = [seen_by([0, 1, 2, 3]), seen_by([0, 2])]
    return vote_case(4, pts, [0] * n, [[0, 1] if f else [] for f in fl], th=2)


def seam_cull(cases):
    """covis_cull_eval: key frame i's slots follow the flags of case i -- a flagged slot holds a point of its own that three key frames outside the list see as well, the
    others are empty -- so nMPs and nRedundant are sums over threads of which the flagged ones hold 1."""
    n_local = len(cases)
    pts, slots = [], []
    for kf, (_, _, fl) in enumerate(cases):
        slots.append([len(pts) + int(fl[:j].sum()) if f else -1 for j, f in enumerate(fl)])
        pts += [seen_by([kf, n_local, n_local + 1, n_local + 2]) for _ in range(int(fl.sum()))]
    return cull_case(n_local + 3, pts, list(range(n_local)), slots)


CASES = {f.__name__: f for f in (vote_threshold, vote_fallback_tie, vote_sort_ties, vote_self_and_skips, vote_double_slot, vote_empty, vote_tile_seam, cull_boundary,
                                 cull_level_seam, cull_depth_and_dynamic, cull_erase_unmakes, cull_erase_makes, cull_not_erase, cull_stereo_decrement, cull_id0, mpcull_cases)}
for _seed in RANDOM_SIZES:
    CASES["random_vote_%d" % _seed] = functools.partial(random_vote, _seed)
    CASES["random_cull_%d" % _seed] = functools.partial(random_cull, _seed)
    CASES["random_mpcull_%d" % _seed] = functools.partial(random_mpcull, _seed)
NAMES = sorted(CASES)
VOTE_NAMES, CULL_NAMES, MPCULL_NAMES = ([n for n in NAMES if k in n.split("_")[:2]] for k in ("vote", "cull", "mpcull"))


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def flat_vote(results):
    """The restatement's per-query results in the layout of cs_covisibility_update."""
    i32 = lambda v: np.array(v, np.int32).reshape(-1)
    cnt_off = np.concatenate([[0], np.cumsum([len(r["counter"]) for r in results])]).astype(np.int32)
    ord_off = np.concatenate([[0], np.cumsum([len(r["ordered"]) for r in results])]).astype(np.int32)
    return dict(cnt_off=cnt_off, cnt_kf=i32([kf for r in results for kf, _ in r["counter"]]), cnt_w=i32([w for r in results for _, w in r["counter"]]),
                kf_max=i32([r["kf_max"] for r in results]), w_max=i32([r["w_max"] for r in results]), ord_off=ord_off,
                ord_kf=i32([kf for r in results for kf, _ in r["ordered"]]), ord_w=i32([w for r in results for _, w in r["ordered"]]))


VOTE_KEYS = ("cnt_off", "cnt_kf", "cnt_w", "kf_max", "w_max", "ord_off", "ord_kf", "ord_w")
CULL_KEYS = ("verdict", "n_mps", "n_redundant", "mp_nobs", "mp_flags", "alive")


@functools.lru_cache(maxsize=None)
def expected(name, skip_dynamic=None):
    """The restatement's answer for a case (a vote case: for one of its skip_dynamic values).  Computed once; do not write to it."""
    c = case(name)
    if c["kind"] == "vote":
        return flat_vote(R.update_connections(c["t"], c["query_kf"], c["kf_off"], c["kf_mp"], skip_dynamic, c["th"]))
    if c["kind"] == "cull":
        return R.keyframe_culling(c["t"], c["local_kf"], c["kf_off"], c["kf_mp"], c["slot_octave"], c["slot_depth"], c["kf_th_depth"], c["monocular"], c["kf_flags"], c["th_obs"])
    return R.mappoint_culling(c["t"], c["recent"], c["mp_found"], c["mp_visible"], c["mp_first_kf_id"], c["current_kf_id"], c["th_obs"])


def obs_table(t):
    from cube_slam_amd.covisibility import ObsTable
    return ObsTable(t["n_kf"], t["obs_off"], t["obs_kf"], t["obs_octave"], t["obs_stereo"], t["mp_nobs"], t["mp_flags"])


def run_vote(ctx, c, skip_dynamic, conn_cap=None):
    from cube_slam_amd.covisibility import covisibility_update
    return covisibility_update(ctx, obs_table(c["t"]), c["query_kf"], c["kf_off"], c["kf_mp"], skip_dynamic, c["th"], conn_cap)


def run_cull(ctx, c):
    from cube_slam_amd.covisibility import KeyFrameCulling
    return KeyFrameCulling(ctx, obs_table(c["t"]), c["local_kf"], c["kf_off"], c["kf_mp"], c["slot_octave"], c["slot_depth"], c["kf_th_depth"], c["monocular"], c["kf_flags"], c["th_obs"])


def run_mpcull(ctx, c):
    from cube_slam_amd.covisibility import MapPointCulling
    return MapPointCulling(ctx, obs_table(c["t"]), c["recent"], c["mp_found"], c["mp_visible"], c["mp_first_kf_id"], c["current_kf_id"], c["th_obs"])


def assert_equal(got, want, keys, what):
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), "%s: %s differs" % (what, k)
        assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype, "%s: dtype of %s" % (what, k)


def dump(c, skip_dynamic=None):
    """A case as the bytes tests/cpp/covisibility_driver.cpp and covisibility_mirror.cpp read: int32 words, byte arrays padded to whole words."""
    words = []
    def i32(v): words.append(np.asarray(v, np.int32).reshape(-1).tobytes())
    def u8(v):
        b = np.asarray(v, np.uint8).reshape(-1).tobytes()
        words.append(b + b"\0" * (-len(b) % 4))
    def f32(v): words.append(np.asarray(v, np.float32).reshape(-1).tobytes())
    t = c["t"]
    i32([{"vote": 0, "cull": 1, "mpcull": 2}[c["kind"]], t["n_kf"], t["n_points"], len(t["obs_kf"])])
    i32(t["obs_off"]); i32(t["obs_kf"]); i32(t["obs_octave"]); u8(t["obs_stereo"]); i32(t["mp_nobs"]); u8(t["mp_flags"])
    if c["kind"] == "vote":
        i32([len(c["query_kf"]), len(c["kf_mp"]), skip_dynamic, c["th"]]); i32(c["query_kf"]); i32(c["kf_off"]); i32(c["kf_mp"])
    elif c["kind"] == "cull":
        i32([len(c["local_kf"]), len(c["kf_mp"]), c["monocular"], c["th_obs"]]); i32(c["local_kf"]); i32(c["kf_off"]); i32(c["kf_mp"]); i32(c["slot_octave"]); f32(c["slot_depth"])
        f32(c["kf_th_depth"]); u8(c["kf_flags"])
    else:
        i32([len(c["recent"]), c["current_kf_id"], c["th_obs"]]); i32(c["recent"]); i32(c["mp_found"]); i32(c["mp_visible"]); i32(c["mp_first_kf_id"])
    return b"".join(words)


def expected_bytes(c, want):
    """What the drivers write for a case: every output array as int32 words, in the order of VOTE_KEYS / CULL_KEYS."""
    keys = VOTE_KEYS if c["kind"] == "vote" else CULL_KEYS if c["kind"] == "cull" else None
    arrays = [want] if keys is None else [want[k] for k in keys]
    return b"".join(np.asarray(a).astype(np.int32).tobytes() for a in arrays)
