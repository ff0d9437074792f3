"""CPU: the host plan of the object BA (cube_slam_amd/csrc/ba_plan.h: argument checks, landmark sort and shard, Schur slots and trips, band plan,
elimination order and symbolic factor, slot order), compiled with g++ into tests/cpp/ba_plan_driver.cpp and run on every graph of ba_patterns.CASES.
What cs_ba_create uploads is exactly what this plans; here its structure is checked against the graph itself, without a device or an oracle."""
import os
import subprocess

import numpy as np
import pytest

from tests import ba_patterns as bp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS_OK, CS_ERR_BAD_ARG, CS_ERR_CAPACITY = 0, -2, -4
BAND_MAX = 20
# the pointers of cs_ba_problem in the order of the driver's null_mask
POINTERS = ("cam_pose", "cam_fixed", "points", "cuboid_pose", "cuboid_scale", "cuboid_flags", "obs_cam", "obs_point", "obs_uv", "obs_inv_sigma2", "cobs_cam", "cobs_cuboid",
            "cobs_bbox", "cobs_info", "pc_cuboid", "pc_offsets", "pc_points")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ba_plan") / "ba_plan_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "ba_plan_driver.cpp"), "-o", str(exe)])
    return str(exe), str(exe.parent)


def write_problem(path, d, null=()):
    """the driver's input: the counts and the arrays the plan reads (see tests/cpp/ba_plan_driver.cpp)"""
    i32 = lambda k: np.ascontiguousarray(d[k], np.int32).reshape(-1)
    f64 = lambda k: np.ascontiguousarray(d[k], np.float64).reshape(-1)
    n_pc = len(d["pc_cuboid"])
    has_ur = d.get("obs_ur") is not None
    head = np.array([len(d["cam_fixed"]), len(d["points"]), len(d["cuboid_pose"]), len(d["obs_cam"]), len(d["cobs_cam"]), n_pc, int(has_ur),
                     sum(1 << POINTERS.index(k) for k in null)], np.int32)
    with open(path, "wb") as f:
        for a in [head, i32("cam_fixed"), i32("obs_cam"), i32("obs_point"), f64("obs_uv"), f64("obs_inv_sigma2")] + ([f64("obs_ur")] if has_ur else []) + \
                 [i32("cobs_cam"), i32("cobs_cuboid"), i32("pc_cuboid")] + ([i32("pc_offsets")] if n_pc else []):
            f.write(a.tobytes())


def plan(driver, d, rank=0, world=1, choice="none", null=()):
    """runs the driver; scalars as ints, arrays as numpy arrays, 'err' the message of a refused build"""
    exe, tmp = driver
    path = os.path.join(tmp, "problem.bin")
    write_problem(path, d, null)
    out = subprocess.run([exe, path, str(rank), str(world), choice], check=True, capture_output=True, text=True).stdout
    X = {}
    for line in out.splitlines():
        kind, name, rest = line.split(" ", 2)
        if kind == "s":
            X[name] = int(rest)
        elif kind == "e":
            X["err"] = name + " " + rest
        else:
            tok = rest.split()
            assert int(tok[0]) == len(tok) - 1
            X[name] = np.array(tok[1:], np.int64) if kind == "i" else np.array([float.fromhex(t) for t in tok[1:]])
    return X


_graphs, _plans = {}, {}


def graph(name):
    if name not in _graphs:
        _graphs[name] = bp.build(name)
    return _graphs[name]


def planned(driver, name):
    """the plan of a graph of CASES on one rank, the library's own choice of solver; computed once"""
    if name not in _plans:
        _plans[name] = plan(driver, graph(name))
        assert _plans[name]["check"] == CS_OK and _plans[name]["build"] == CS_OK
    return _plans[name]


ALL = sorted(bp.CASES)


@pytest.mark.parametrize("name", ALL)
def test_band_shape_and_path(driver, name):
    """(C, Bc) as the library plans them are what ba_patterns.band_shape restates and what each graph is built to have; the path follows from them"""
    X, d = planned(driver, name), graph(name)
    assert (X["C"], X["graph_bc"]) == bp.CASES[name][1] == bp.band_shape(d)
    assert X["band_bc"] == (max(X["graph_bc"], 1) if X["use_band"] else 0)
    assert bool(X["use_band"]) == (X["C"] >= 1 and X["graph_bc"] <= BAND_MAX)
    assert bool(X["band_twist"]) == (bool(X["use_band"]) and X["C"] >= 6 * (X["band_bc"] + 1))
    assert X["P"] == X["C"] + X["Q"] and X["Q"] == len(d["cuboid_pose"]) and np.array_equal(X["cam_idx"], bp.free_index(d))


def test_paths_at_their_thresholds(driver):
    for choice in ("band", "band1"):
        X = plan(driver, graph("ladder_Bc21"), choice=choice)
        assert X["check"] == CS_OK and X["build"] == CS_ERR_CAPACITY and "not narrow-banded" in X["err"]
    assert not planned(driver, "ladder_Bc21")["use_band"] and planned(driver, "ladder_Bc20")["use_band"]
    assert not planned(driver, "all_fixed_cuboids_only")["use_band"]  # no free camera: the sparse path
    assert not planned(driver, "twist_C29_Bc4")["band_twist"] and planned(driver, "twist_C30_Bc4")["band_twist"]
    assert planned(driver, "long_Bc20")["band_twist"]
    X = plan(driver, graph("twist_C30_Bc4"), choice="band1")
    assert X["use_band"] and not X["band_twist"]
    X = plan(driver, graph("twist_C30_Bc4"), choice="sparse")
    assert not X["use_band"] and len(X["tgt_slot"]) == 0


def _check_sort_and_shard(X, d):
    n_obs, pt, cam = len(d["obs_cam"]), np.asarray(d["obs_point"], np.int64), np.asarray(d["obs_cam"], np.int64)
    perm = X["obs_perm"]
    assert np.array_equal(np.sort(perm), np.arange(n_obs))
    assert np.array_equal(perm, np.argsort(pt, kind="stable"))  # by landmark, the caller's order kept inside a landmark
    assert np.array_equal(X["o_pt"], pt[perm]) and np.array_equal(X["o_cam"], cam[perm])
    assert np.array_equal(X["o_uv"], np.asarray(d["obs_uv"], np.float64)[perm].reshape(-1)) and np.array_equal(X["o_w"], np.asarray(d["obs_inv_sigma2"], np.float64)[perm])
    assert np.array_equal(X["lm_off"], np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=len(d["points"])))]))
    assert (X["o_b"], X["o_e"]) == (X["lm_off"][X["lm_b"]], X["lm_off"][X["lm_e"]])
    # every observation of a free camera in the rank's range once, ascending per pose block
    q = np.arange(X["o_b"], X["o_e"])
    pi = X["cam_idx"][X["o_cam"][q]]
    q, pi = q[pi >= 0], pi[pi >= 0]
    assert np.array_equal(X["pose_off"], np.concatenate([[0], np.cumsum(np.bincount(pi, minlength=X["P"]))]))
    assert np.array_equal(X["pose_obs"][:len(q)], q[np.argsort(pi, kind="stable")])


def _live_trips(X):
    """(slot of every trip, trips) without the dummy entry of an empty list"""
    n = X["slot_off"][-1]
    return np.repeat(np.arange(X["n_slots"]), np.diff(X["slot_off"])), X["trips"].reshape(-1, 2)[:n]


def _check_slots(X, d):
    P, C, n_cobs = X["P"], X["C"], len(d["cobs_cam"])
    rc = X["slot_rc"].reshape(-1, 2)
    assert len(rc) == X["n_slots"] and np.array_equal(rc[:P], np.stack([np.arange(P)] * 2, axis=1))
    ci = X["cam_idx"][np.asarray(d["cobs_cam"], np.int64)]
    want = np.stack([ci, C + np.asarray(d["cobs_cuboid"], np.int64)], axis=1)
    want[ci < 0] = -1  # a fixed camera's edge: dead block
    assert np.array_equal(rc[P:P + n_cobs], want)
    cc = rc[P + n_cobs:]  # camera-camera blocks made by shared landmarks
    assert (cc[:, 0] < cc[:, 1]).all() and (cc[:, 1] < C).all() and (cc[:, 0] >= 0).all() and len(np.unique(cc, axis=0)) == len(cc)
    slot, trips = _live_trips(X)
    u, v = trips[:, 0], trips[:, 1]
    assert np.array_equal(X["o_pt"][u], X["o_pt"][v])
    assert np.array_equal(np.stack([X["cam_idx"][X["o_cam"][u]], X["cam_idx"][X["o_cam"][v]]], axis=1), rc[slot])
    assert ((X["o_pt"][u] >= X["lm_b"]) & (X["o_pt"][u] < X["lm_e"])).all()
    q = np.arange(X["o_b"], X["o_e"])
    k = np.bincount(X["o_pt"][q][X["cam_idx"][X["o_cam"][q]] >= 0], minlength=1)  # free-camera observations per landmark of the rank
    assert len(trips) == int((k * (k + 1) // 2).sum())
    assert len(np.unique(trips, axis=0)) == len(trips)
    assert np.array_equal(np.sort(X["slot_perm"]), np.arange(X["n_slots"]))
    assert X["reduce_len"] == X["n_slots"] * 36 + P * 6


def _check_factor(X):
    P, rc = X["P"], X["slot_rc"].reshape(-1, 2)
    assert np.array_equal(np.sort(X["pos"]), np.arange(P))
    n_rows = X["col_off"][-1]
    assert X["band_len"] == (P + n_rows) * 36
    for k in range(P):
        r = X["rows"][X["col_off"][k]:X["col_off"][k + 1]]
        assert (np.diff(r) > 0).all() and (r > k).all() and (r < P).all()
    m = np.diff(X["col_off"])
    assert np.array_equal(X["pair_off"], np.concatenate([[0], np.cumsum(m * (m + 1) // 2)])) and X["max_col"] == (m.max() if P else 0)
    assert (X["upd_tgt"] >= 0).all() and (X["upd_tgt"] < P + max(n_rows, 1)).all()  # fill-in is closed
    live = rc[:, 0] >= 0
    dst = X["slot_dst"]
    assert (dst[~live] == -1).all() and (dst[live] >= 0).all() and (dst[live] < P + len(X["rows"])).all() and (dst[live] < P + max(n_rows, 1)).all()
    assert len(np.unique(dst[live])) == live.sum()
    # a slot's block sits where the elimination order puts it: below the diagonal of the earlier column, transposed when its rows come first
    a, c = X["pos"][rc[live, 0]], X["pos"][rc[live, 1]]
    assert np.array_equal(X["slot_tr"][live], (a < c).astype(int)) and (X["slot_tr"][~live] == 0).all()
    off = dst[live] >= P
    col = np.searchsorted(X["col_off"], dst[live][off] - P, side="right") - 1
    assert np.array_equal(col, np.minimum(a, c)[off]) and np.array_equal(X["rows"][dst[live][off] - P], np.maximum(a, c)[off]) and np.array_equal(dst[live][~off], a[~off])


def _check_band(X, d):
    if not X["use_band"]:
        return
    P, C, Q, Bc, n_cobs = X["P"], X["C"], X["Q"], X["band_bc"], len(d["cobs_cam"])
    rc = X["slot_rc"].reshape(-1, 2)
    assert X["band_targets"] == C * (Bc + 1) == len(X["tgt_slot"]) == len(X["tgt_tr"])
    s = np.arange(X["n_slots"])
    camcam = (rc[:, 0] >= 0) & (rc[:, 0] < C) & (rc[:, 1] < C) & ((s < P) | (s >= P + n_cobs))
    at = np.minimum(rc[camcam, 0], rc[camcam, 1]) * (Bc + 1) + np.abs(rc[camcam, 0] - rc[camcam, 1])
    assert np.array_equal(X["tgt_slot"][at], s[camcam]) and (X["tgt_slot"] >= 0).sum() == camcam.sum()  # each once, at (min, |i - j|)
    assert np.array_equal(X["tgt_tr"][at], (rc[camcam, 0] < rc[camcam, 1]).astype(int))
    ci = X["cam_idx"][np.asarray(d["cobs_cam"], np.int64)]
    cq = np.asarray(d["cobs_cuboid"], np.int64)
    assert np.array_equal(X["cq_off"], np.concatenate([[0], np.cumsum(np.bincount(cq[ci >= 0], minlength=Q))]))  # CSR over the cuboids' live edges
    lst = X["cq_list"].reshape(-1, 2)[:X["cq_off"][-1]]  # (slot, camera)
    for q in range(Q):
        e = np.nonzero((cq == q) & (ci >= 0))[0]
        e = e[np.argsort(ci[e], kind="stable")]
        assert np.array_equal(lst[X["cq_off"][q]:X["cq_off"][q + 1]], np.stack([P + e, ci[e]], axis=1))
    assert X["cr_off"][-1] == X["cq_off"][-1] and len(X["cr_off"]) == C + 1 and len(X["ct_off"]) == C * (Bc + 1) + 1


@pytest.mark.parametrize("name", ALL)
def test_plan_structure(driver, name):
    X, d = planned(driver, name), graph(name)
    _check_sort_and_shard(X, d)
    _check_slots(X, d)
    _check_factor(X)
    _check_band(X, d)
    if len(d["cobs_cam"]) + len(d["pc_cuboid"]):  # pose edges: every edge once per vertex it touches
        assert X["pe_off"][-1] == (X["cam_idx"][np.asarray(d["cobs_cam"], np.int64)] >= 0).sum() + len(d["cobs_cam"]) + len(d["pc_cuboid"])


def test_sharding_three_ranks(driver):
    """the slot pattern is the same on every rank; the trips are split by landmark; the pose edges live on rank 0"""
    d = graph("chain30_cub4")
    one = planned(driver, "chain30_cub4")
    ranks = [plan(driver, d, rank=r, world=3) for r in range(3)]
    s1, t1 = _live_trips(one)
    per_slot = [[] for _ in range(one["n_slots"])]
    for r, X in enumerate(ranks):
        assert X["build"] == CS_OK
        _check_sort_and_shard(X, d); _check_slots(X, d); _check_factor(X); _check_band(X, d)
        for k in ("n_slots", "slot_rc", "slot_dst", "slot_tr", "slot_perm", "pos", "rows", "tgt_slot", "use_band", "band_bc"):
            assert np.array_equal(X[k], one[k]), k
        assert (X["lm_b"], X["lm_e"]) == (len(d["points"]) * r // 3, len(d["points"]) * (r + 1) // 3)
        s, t = _live_trips(X)
        for i in range(one["n_slots"]):
            per_slot[i].append(t[s == i])
    assert ranks[0]["lm_b"] == 0 and ranks[2]["lm_e"] == len(d["points"]) and all(X["lm_e"] > X["lm_b"] for X in ranks)
    for i in range(one["n_slots"]):
        assert np.array_equal(np.concatenate(per_slot[i]), t1[s1 == i]), i
    # pose edges exist only on rank 0: the incidence lists do not depend on the shard and are planned alike everywhere, pose_edges says whose kernels read them
    assert [X["pose_edges"] for X in ranks] == [1, 0, 0] and one["pose_edges"] == 1
    assert all(np.array_equal(X["pe_list"], one["pe_list"]) and np.array_equal(X["pe_off"], one["pe_off"]) for X in ranks)


def _with_cuboid(d):
    """tiny_kf3 has no cuboid: one cuboid with one camera-cuboid edge (camera 1) and one point-cuboid edge of two points, for the edits of those edges"""
    d2 = dict(d)
    d2.update(cuboid_pose=np.array([[0, 0, 10.0, 0, 0, 0, 1]]), cuboid_scale=np.ones((1, 3)), cuboid_flags=np.zeros(1, np.uint8), cobs_cam=np.array([1], np.int32),
              cobs_cuboid=np.array([0], np.int32), cobs_bbox=np.array([[100.0, 100, 200, 200]]), cobs_info=np.ones((1, 4)), pc_cuboid=np.array([0], np.int32),
              pc_offsets=np.array([0, 2], np.int32), pc_points=np.zeros((2, 3)))
    return d2


def _edit(d, key, index, value):
    d2 = dict(d)
    a = np.array(d[key]).copy()
    a[index] = value
    d2[key] = a
    return d2


def test_malformed_problems_are_refused(driver):
    base = graph("tiny_kf3")
    cub = _with_cuboid(base)
    assert plan(driver, base)["check"] == CS_OK and plan(driver, cub)["build"] == CS_OK
    n_cams, n_pts = len(base["cam_fixed"]), len(base["points"])
    bad = {}
    for v, tag in ((-1, "minus one"), (None, "one past the end")):
        bad["obs_cam " + tag] = _edit(base, "obs_cam", 5, n_cams if v is None else v)
        bad["obs_point " + tag] = _edit(base, "obs_point", 5, n_pts if v is None else v)
        bad["cobs_cam " + tag] = _edit(cub, "cobs_cam", 0, n_cams if v is None else v)
        bad["cobs_cuboid " + tag] = _edit(cub, "cobs_cuboid", 0, 1 if v is None else v)
        bad["pc_cuboid " + tag] = _edit(cub, "pc_cuboid", 0, 1 if v is None else v)
    bad["pc_offsets[0] = 1"] = _edit(cub, "pc_offsets", 0, 1)
    bad["pc_offsets decreasing"] = _edit(cub, "pc_offsets", 1, -1)
    bad["every camera fixed, no cuboid"] = bp.fix_cameras(base, range(n_cams))
    for tag, d in bad.items():
        assert plan(driver, d)["check"] == CS_ERR_BAD_ARG, tag
    assert plan(driver, base, null=("cam_fixed",))["check"] == CS_ERR_BAD_ARG
    assert plan(driver, base, null=("obs_uv",))["check"] == CS_ERR_BAD_ARG
    for r, w in ((-1, 1), (1, 1), (0, 0)):
        assert plan(driver, base, rank=r, world=w)["check"] == CS_ERR_BAD_ARG
    assert plan(driver, bp.fix_cameras(cub, range(n_cams)))["build"] == CS_OK  # a cuboid alone is a vertex to solve for


def test_zero_size_problem(driver):
    """no landmark and no observation, the cuboid edges kept: `points` is NULL in the driver, so a plan that read it would not come back"""
    d = dict(bp.chain14())
    for k in ("obs_cam", "obs_point", "obs_uv", "obs_inv_sigma2", "points"):
        d[k] = np.asarray(d[k])[:0]
    X = plan(driver, d)
    assert X["check"] == CS_OK and X["build"] == CS_OK and (X["lm_b"], X["lm_e"], X["o_b"], X["o_e"]) == (0, 0, 0, 0)
    _check_sort_and_shard(X, d); _check_slots(X, d); _check_factor(X); _check_band(X, d)
    assert X["n_slots"] == X["P"] + len(d["cobs_cam"]) and X["slot_off"][-1] == 0 and len(X["trips"]) == 2  # no trip but the dummy
    assert X["pe_off"][-1] == (X["cam_idx"][np.asarray(d["cobs_cam"], np.int64)] >= 0).sum() + len(d["cobs_cam"]) + len(d["pc_cuboid"]) > 0
