"""GPU: the graph work of one local-mapping cycle as a chain on one seeded map, each stage's output tables feeding the next: a new key frame's observations are added and
UpdateConnections runs; MapPointCulling runs and its bad flags are applied; KeyFrameCulling runs.  Equal, stage by stage, to the restatement run as one sequence."""
import numpy as np
import pytest

from tests import covisibility_patterns as P
from tests import covisibility_restatement as R

pytestmark = pytest.mark.gpu


def _with_new_keyframe(m, rng):
    """ProcessNewKeyFrame's AddObservation calls: key frame n_kf sees every third point that is not bad (its index is the highest, so the runs stay ascending)."""
    new = m["n_kf"]
    pts, slots, octaves = [dict(p, obs=list(p["obs"])) for p in m["points"]], [], []
    for p in range(0, len(pts), 3):
        if pts[p].get("flags", 0) & 1:
            continue
        stereo = int(rng.random() < 0.3)
        level = int(rng.integers(1, 6))
        if "nobs" in pts[p]:
            pts[p]["nobs"] += 1
        pts[p]["obs"].append((new, level, stereo))
        slots.append(p); octaves.append(level)
    return pts, slots + [-1, -1], octaves + [0, 0]


def _table_dict(t):
    return dict(n_kf=t.n_kf, n_points=t.n_points, obs_off=t.obs_off, obs_kf=t.obs_kf, obs_octave=t.obs_octave, obs_stereo=t.obs_stereo, mp_nobs=t.mp_nobs, mp_flags=t.mp_flags)


def _restated_after_mpcull(t, recent, cases):
    """MapPoint::SetBadFlag for cases 2 and 3, on dictionaries."""
    m = R.Map(t)
    for p, c in zip(recent.tolist(), cases.tolist()):
        if c in (2, 3):
            m.SetBadFlag(p)
    nobs, flags, alive = m.state()
    keep = alive.astype(bool)
    off = np.concatenate([[0], np.cumsum(keep)])[t["obs_off"]].astype(np.int32)
    return dict(t, obs_off=off, obs_kf=t["obs_kf"][keep], obs_octave=t["obs_octave"][keep], obs_stereo=t["obs_stereo"][keep], mp_nobs=nobs, mp_flags=flags)


def test_cycle_chain(ctx):
    from cube_slam_amd.covisibility import Connections, KeyFrameCulling, MapPointCulling, UpdateConnections, apply_mappoint_cases
    m = P.random_map(0)
    rng = np.random.default_rng(77)
    pts, new_slots, new_octaves = _with_new_keyframe(m, rng)
    new, n_kf = m["n_kf"], m["n_kf"] + 1
    t0 = P.table(n_kf, pts)
    slots, octaves, depths = m["slots"] + [new_slots], m["octaves"] + [new_octaves], m["depths"] + [[1.0] * len(new_slots)]
    kf_off, kf_mp = P.lists(slots)

    # 1. UpdateConnections: every old key frame first (the state the map is in), then the new one
    table = P.obs_table(t0)
    conn, order = Connections(n_kf), list(range(n_kf))
    r1 = UpdateConnections(ctx, table, order, kf_off, kf_mp, conn, skip_dynamic=True, th=15)
    want1 = R.update_connections(t0, order, kf_off, kf_mp, 1, 15)
    P.assert_equal(r1, P.flat_vote(want1), P.VOTE_KEYS, "UpdateConnections")
    assert conn.snapshot() == R.apply_connections(n_kf, order, want1)
    local = conn.ordered_kf[new]  # GetVectorCovisibleKeyFrames of the new key frame: KeyFrameCulling's list
    assert len(local) >= 10 and conn.parent[new] == local[0]

    # 2. MapPointCulling over the recent list, then its SetBadFlag calls
    recent = np.arange(0, t0["n_points"], 5, dtype=np.int32)
    cases = MapPointCulling(ctx, table, recent, m["found"], m["visible"], m["first"], current_kf_id=6, th_obs=3)
    want_cases = R.mappoint_culling(t0, recent, m["found"], m["visible"], m["first"], 6, 3)
    assert np.array_equal(cases, want_cases) and {2, 3} <= set(cases.tolist())
    table2, remaining = apply_mappoint_cases(table, recent, cases)
    t2 = _restated_after_mpcull(t0, recent, want_cases)
    assert all(np.array_equal(v, t2[k]) for k, v in _table_dict(table2).items()) and np.array_equal(remaining, recent[want_cases == 0])

    # 3. KeyFrameCulling over the new key frame's covisibles, on the table stage 2 left
    pick = lambda v: [v[k] for k in local]
    off3, mp3 = P.lists(pick(slots))
    oct3, dep3 = np.concatenate(pick(octaves)).astype(np.int32), np.concatenate(pick(depths)).astype(np.float32)
    th_depth, flags = np.full(len(local), 40.0, np.float32), np.array([1 if k == 0 else 0 for k in local], np.uint8)
    r3 = KeyFrameCulling(ctx, table2, local, off3, mp3, oct3, dep3, th_depth, False, flags, th_obs=3)
    want3 = R.keyframe_culling(t2, local, off3, mp3, oct3, dep3, th_depth, 0, flags, 3)
    P.assert_equal(r3, want3, P.CULL_KEYS, "KeyFrameCulling")
    assert (want3["verdict"] == 1).sum() >= 2 and r3["n_rounds"] >= 3
