"""GPU: cs_covisibility_update, cs_keyframe_culling and cs_mappoint_culling on the device, through the C-ABI and the Python mirror, equal to the restatement
(tests/covisibility_restatement.py) on every pattern.  Everything is integers: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from tests import covisibility_patterns as P
from tests import covisibility_restatement as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", P.VOTE_NAMES)
def test_vote(ctx, name):
    c = P.case(name)
    for sd in c["skip_dynamic"]:
        P.assert_equal(P.run_vote(ctx, c, sd), P.expected(name, sd), P.VOTE_KEYS, "%s skip_dynamic=%d" % (name, sd))


@pytest.mark.parametrize("name", P.CULL_NAMES)
def test_cull(ctx, name):
    got, want = P.run_cull(ctx, P.case(name)), P.expected(name)
    P.assert_equal(got, want, P.CULL_KEYS, name)
    n, erased = len(want["verdict"]), np.flatnonzero(want["verdict"] == 1)
    assert got["n_rounds"] == len(erased) + (0 if len(erased) and erased[-1] == n - 1 else 1)  # a round per erasing key frame and one that finds none


@pytest.mark.parametrize("name", P.MPCULL_NAMES)
def test_mpcull(ctx, name):
    got = P.run_mpcull(ctx, P.case(name))
    assert got.dtype == np.uint8 and np.array_equal(got, P.expected(name))


def _vote_want(c):
    return P.flat_vote(R.update_connections(c["t"], c["query_kf"], c["kf_off"], c["kf_mp"], 1, c["th"]))


def test_scan_seams(ctx):
    """The workgroup-wide scans under covis_vote (over the threads' counters), covis_offsets (over the queries) and covis_cull_eval (its two sums over the slots) at the
    seams of a wave and of a pass of 256 threads, nothing and everything flagged: tests/compaction_seams.py through P.seam_*."""
    from tests import compaction_seams as cs
    cases = cs.cases()
    for n, pattern, fl in cases:
        c = P.seam_vote_counters(n, fl)
        got = P.run_vote(ctx, c, 1)
        P.assert_equal(got, _vote_want(c), P.VOTE_KEYS, "counters %d %s" % (n, pattern))
        assert got["cnt_kf"].tolist() == [P.PER_THREAD * int(i) + int(i) % P.PER_THREAD for i in np.flatnonzero(fl)]
        c = P.seam_vote_queries(n, fl)
        got = P.run_vote(ctx, c, 1)
        P.assert_equal(got, _vote_want(c), P.VOTE_KEYS, "queries %d %s" % (n, pattern))
        assert np.diff(got["cnt_off"]).tolist() == [3 if f else 0 for f in fl] and np.diff(got["ord_off"]).tolist() == [1 if f else 0 for f in fl]
    c = P.seam_cull(cases)
    got = P.run_cull(ctx, c)
    want = R.keyframe_culling(c["t"], c["local_kf"], c["kf_off"], c["kf_mp"], c["slot_octave"], c["slot_depth"], c["kf_th_depth"], c["monocular"], c["kf_flags"], c["th_obs"])
    P.assert_equal(got, want, P.CULL_KEYS, "cull")
    assert got["n_mps"].tolist() == got["n_redundant"].tolist() == [int(fl.sum()) for _, _, fl in cases]


def test_c_abi_directly(ctx):
    """The three entry points with nothing of the Python mirror between: buffers sized by hand, canaries behind every output."""
    from cube_slam_amd._lib import lib, ptr
    c, want = P.case("random_vote_1"), P.expected("random_vote_1", 1)
    t = P.obs_table(c["t"])
    s = t.c_struct()
    nq, cap = len(c["query_kf"]), int(want["cnt_off"][-1])
    i32 = lambda n: np.full(n + 3, -77, np.int32)
    cnt_off, ord_off, kf_max, w_max, cnt_kf, cnt_w, ord_kf, ord_w = i32(nq + 1), i32(nq + 1), i32(nq), i32(nq), i32(cap), i32(cap), i32(cap), i32(cap)
    r = lib().cs_covisibility_update(ctx.ptr, C.byref(s), nq, ptr(c["query_kf"]), ptr(c["kf_off"]), ptr(c["kf_mp"]), 1, c["th"], cap, ptr(cnt_off), ptr(cnt_kf), ptr(cnt_w),
                                     ptr(kf_max), ptr(w_max), ptr(ord_off), ptr(ord_kf), ptr(ord_w))
    assert r == 0
    for got, key in ((cnt_off, "cnt_off"), (cnt_kf, "cnt_kf"), (cnt_w, "cnt_w"), (kf_max, "kf_max"), (w_max, "w_max"), (ord_off, "ord_off"), (ord_kf, "ord_kf"), (ord_w, "ord_w")):
        n = len(want[key])
        assert np.array_equal(got[:n], want[key]) and (got[n:] == -77).all(), key

    c, want = P.case("random_cull_1"), P.expected("random_cull_1")
    t = P.obs_table(c["t"])
    s = t.c_struct()
    nl = len(c["local_kf"])
    u8 = lambda n: np.full(n + 3, 0xAB, np.uint8)
    verdict, flags, alive, n_mps, n_red, nobs = u8(nl), u8(t.n_points), u8(t.n_obs), i32(nl), i32(nl), i32(t.n_points)
    before = [a.copy() for a in (t.mp_nobs, t.mp_flags, t.obs_kf)]
    r = lib().cs_keyframe_culling(ctx.ptr, C.byref(s), nl, ptr(c["local_kf"]), ptr(c["kf_off"]), ptr(c["kf_mp"]), ptr(c["slot_octave"]), ptr(c["slot_depth"]), ptr(c["kf_th_depth"]),
                                  c["monocular"], ptr(c["kf_flags"]), c["th_obs"], ptr(verdict), ptr(n_mps), ptr(n_red), ptr(nobs), ptr(flags), ptr(alive), None)
    assert r == 0
    for got, key, canary in ((verdict, "verdict", 0xAB), (n_mps, "n_mps", -77), (n_red, "n_redundant", -77), (nobs, "mp_nobs", -77), (flags, "mp_flags", 0xAB), (alive, "alive", 0xAB)):
        n = len(want[key])
        assert np.array_equal(got[:n], want[key]) and (got[n:] == canary).all(), key
    assert all(np.array_equal(a, b) for a, b in zip(before, (t.mp_nobs, t.mp_flags, t.obs_kf))), "the caller's tables are inputs"

    c, want = P.case("random_mpcull_1"), P.expected("random_mpcull_1")
    t = P.obs_table(c["t"])
    s = t.c_struct()
    cases = u8(len(c["recent"]))
    r = lib().cs_mappoint_culling(ctx.ptr, C.byref(s), len(c["recent"]), ptr(c["recent"]), ptr(c["mp_found"]), ptr(c["mp_visible"]), ptr(c["mp_first_kf_id"]), c["current_kf_id"],
                                  c["th_obs"], ptr(cases))
    assert r == 0 and np.array_equal(cases[:len(want)], want) and (cases[len(want):] == 0xAB).all()


def test_capacity_fills_cnt_off(ctx):
    from cube_slam_amd._lib import CubeSlamError
    c, want = P.case("random_vote_0"), P.expected("random_vote_0", 1)
    total = int(want["cnt_off"][-1])
    for cap in (0, total - 1):
        with pytest.raises(CubeSlamError) as e:
            P.run_vote(ctx, c, 1, conn_cap=cap)
        assert e.value.status == -4 and np.array_equal(e.value.cnt_off, want["cnt_off"])
    P.assert_equal(P.run_vote(ctx, c, 1, conn_cap=total), want, P.VOTE_KEYS, "exact capacity")


def test_same_call_twice_same_bytes(ctx):
    for name in ("random_vote_0", "vote_tile_seam"):
        a, b = P.run_vote(ctx, P.case(name), 1), P.run_vote(ctx, P.case(name), 1)
        assert all(a[k].tobytes() == b[k].tobytes() for k in P.VOTE_KEYS)
    a, b = P.run_cull(ctx, P.case("random_cull_0")), P.run_cull(ctx, P.case("random_cull_0"))
    assert all(a[k].tobytes() == b[k].tobytes() for k in P.CULL_KEYS) and a["n_rounds"] == b["n_rounds"]
    assert P.run_mpcull(ctx, P.case("random_mpcull_0")).tobytes() == P.run_mpcull(ctx, P.case("random_mpcull_0")).tobytes()


def test_device_and_host_forms_agree(ctx):
    for name in ("random_vote_2", "vote_tile_seam"):
        a, b = P.run_vote(ctx, P.case(name), 0), P.run_vote(None, P.case(name), 0)
        assert all(a[k].tobytes() == b[k].tobytes() for k in P.VOTE_KEYS)
    a, b = P.run_cull(ctx, P.case("random_cull_2")), P.run_cull(None, P.case("random_cull_2"))
    assert all(a[k].tobytes() == b[k].tobytes() for k in P.CULL_KEYS)


def test_bad_arguments_on_the_device_path(ctx):
    """The device entry points refuse what the host forms refuse, before anything is launched."""
    from cube_slam_amd._lib import CubeSlamError
    c = dict(P.case("vote_threshold"))
    c["kf_mp"] = c["kf_mp"].copy()
    c["kf_mp"][3] = c["t"]["n_points"]  # a slot outside the point table
    with pytest.raises(CubeSlamError) as e:
        P.run_vote(ctx, c, 1)
    assert e.value.status == -2
    c = dict(P.case("cull_boundary"))
    c["local_kf"] = c["local_kf"].copy()
    c["local_kf"][0] = c["t"]["n_kf"]
    with pytest.raises(CubeSlamError, match="CS_ERR_BAD_ARG"):
        P.run_cull(ctx, c)


def test_update_connections_mirror(ctx):
    from cube_slam_amd.covisibility import Connections, UpdateConnections
    c = P.case("random_vote_1")
    n_kf, queries = c["t"]["n_kf"], c["query_kf"].tolist()
    conn = Connections(n_kf)
    UpdateConnections(ctx, P.obs_table(c["t"]), queries, c["kf_off"], c["kf_mp"], conn, skip_dynamic=True, th=c["th"])
    assert conn.snapshot() == R.apply_connections(n_kf, queries, R.update_connections(c["t"], queries, c["kf_off"], c["kf_mp"], 1, c["th"]))
