"""CPU: every designed input of tests/covisibility_patterns.py holds what its name says, judged by the restatement (tests/covisibility_restatement.py)."""
from fractions import Fraction

import numpy as np

from tests import covisibility_patterns as P
from tests import covisibility_restatement as R


def _vote(name, skip_dynamic=1):
    c = P.case(name)
    return R.update_connections(c["t"], c["query_kf"], c["kf_off"], c["kf_mp"], skip_dynamic, c["th"])


def test_counter_tile_is_the_kernel_sources():
    from cube_slam_amd import covisibility
    assert covisibility.COUNTER_TILE == covisibility.source_counter_tile() == P.TILE


def test_case_names():
    assert {"vote_threshold", "vote_fallback_tie", "vote_sort_ties", "vote_self_and_skips", "vote_double_slot", "vote_empty", "vote_tile_seam", "cull_boundary", "cull_level_seam",
            "cull_depth_and_dynamic", "cull_erase_unmakes", "cull_erase_makes", "cull_not_erase", "cull_stereo_decrement", "cull_id0", "mpcull_cases"} <= set(P.NAMES)
    assert len(P.VOTE_NAMES) == 10 and len(P.CULL_NAMES) == 11 and len(P.MPCULL_NAMES) == 4
    assert sorted(P.VOTE_NAMES + P.CULL_NAMES + P.MPCULL_NAMES) == P.NAMES


def test_vote_threshold():
    (r,) = _vote("vote_threshold")
    assert r["counter"] == [(1, 14), (2, 15), (3, 16)] and r["ordered"] == [(3, 16), (2, 15)] and (r["kf_max"], r["w_max"]) == (3, 16)


def test_vote_fallback_tie():
    (r,) = _vote("vote_fallback_tie")
    assert r["counter"] == [(1, 2), (2, 3), (4, 3)] and (r["kf_max"], r["w_max"]) == (2, 3) and r["ordered"] == [(2, 3)]


def test_vote_sort_ties():
    (r,) = _vote("vote_sort_ties")
    assert r["ordered"] == [(2, 17), (5, 16), (3, 16), (1, 16)] and r["kf_max"] == 2


def test_vote_self_and_skips():
    (on,), (off,) = _vote("vote_self_and_skips", 1), _vote("vote_self_and_skips", 0)
    assert on["counter"] == [(1, 1)] and off["counter"] == [(1, 1), (2, 1)]
    assert P.case("vote_self_and_skips")["skip_dynamic"] == (1, 0)


def test_vote_double_slot():
    (r,) = _vote("vote_double_slot")
    assert r["counter"] == [(1, 2)]


def test_vote_empty():
    r = _vote("vote_empty")
    assert [x["kf_max"] for x in r] == [-1, -1, 2, -1] and [x["ordered"] for x in r] == [[], [], [(2, 1)], []]
    f = P.expected("vote_empty", 1)
    assert f["cnt_off"].tolist() == [0, 0, 0, 1, 1] and f["w_max"].tolist() == [0, 0, 1, 0]


def test_vote_tile_seam():
    T = P.TILE
    c = P.case("vote_tile_seam")
    assert c["t"]["n_kf"] == 3 * T + 5 and P.SEAM_VOTERS == (T - 1, T, T + 1, 2 * T - 1, 2 * T, 3 * T + 4)
    a, b = _vote("vote_tile_seam")
    assert a["counter"] == [(v, i + 1) for i, v in enumerate(P.SEAM_VOTERS)] and (a["kf_max"], a["w_max"]) == (3 * T + 4, 6)
    assert a["ordered"] == [(v, i + 1) for i, v in reversed(list(enumerate(P.SEAM_VOTERS))) if i + 1 >= 3]
    assert [kf for kf, _ in b["counter"]] == [0] + [v for v in P.SEAM_VOTERS if v != T] and dict(b["counter"])[0] == 6  # the voter at TILE asks: its own index is not counted


def _cull(name, frozen=False):
    c = P.case(name)
    return R.keyframe_culling(c["t"], c["local_kf"], c["kf_off"], c["kf_mp"], c["slot_octave"], c["slot_depth"], c["kf_th_depth"], c["monocular"], c["kf_flags"], c["th_obs"],
                              frozen=frozen)


def test_nine_tenths_is_exact_for_multiples_of_ten():
    """0.9 * n in double is the integer 9 n / 10 for every multiple of 10 up to 2000, so `nRedundant > 0.9 * nMPs` at the boundary is a comparison of integers."""
    for n in range(0, 2001, 10):
        assert Fraction(0.9 * float(n)) == Fraction(9 * n, 10), n


def test_cull_boundary():
    r = _cull("cull_boundary")
    assert r["n_mps"].tolist() == [10, 10, 20, 20] and r["n_redundant"].tolist() == [9, 10, 18, 19] and r["verdict"].tolist() == [0, 1, 0, 1]


def test_cull_level_seam():
    c, r = P.case("cull_level_seam"), _cull("cull_level_seam")
    assert r["n_mps"].tolist() == [5] and r["n_redundant"].tolist() == [2]
    t = c["t"]
    assert t["mp_nobs"].tolist() == [4, 4, 3, 5, 5] and np.diff(t["obs_off"]).tolist() == [4, 4, 4, 4, 3]
    one = lambda p: R.keyframe_culling(t, [0], [0, 1], [p], [2], [1.0], [40.0], 1, [0], 3)["n_redundant"][0]
    assert [one(p) for p in range(5)] == [1, 0, 0, 1, 0]


def test_cull_depth_and_dynamic():
    r = _cull("cull_depth_and_dynamic")
    assert r["n_mps"].tolist() == [3] and r["n_redundant"].tolist() == [3] and r["verdict"].tolist() == [1]  # depth == mThDepth and the two plain points


def test_cull_erase_unmakes():
    seq, frozen = _cull("cull_erase_unmakes"), _cull("cull_erase_unmakes", frozen=True)
    assert frozen["verdict"].tolist() == [1, 1] and frozen["n_redundant"].tolist() == [20, 10]
    assert seq["verdict"].tolist() == [1, 0] and seq["n_redundant"].tolist() == [20, 0] and seq["mp_nobs"][10:].tolist() == [3] * 10
    assert not (seq["mp_flags"] & 1).any()


def test_cull_erase_makes():
    seq, frozen = _cull("cull_erase_makes"), _cull("cull_erase_makes", frozen=True)
    assert frozen["verdict"].tolist() == [1, 0] and (frozen["n_mps"][1], frozen["n_redundant"][1]) == (10, 9)
    assert seq["verdict"].tolist() == [1, 1] and (seq["n_mps"][1], seq["n_redundant"][1]) == (9, 9)
    assert seq["mp_flags"][10] & 1 and seq["mp_nobs"][10] == 2 and not seq["alive"][P.case("cull_erase_makes")["t"]["obs_off"][10]:][:3].any()


def test_cull_not_erase():
    c, r = P.case("cull_not_erase"), _cull("cull_not_erase")
    assert r["verdict"].tolist() == [2, 1] and r["n_redundant"].tolist() == [20, 10]
    assert r["mp_nobs"][:10].tolist() == c["t"]["mp_nobs"][:10].tolist()  # A's own points are untouched; B's erasure shows on the others
    assert r["mp_nobs"][10:].tolist() == [3] * 10


def test_cull_stereo_decrement():
    r = _cull("cull_stereo_decrement")
    assert r["verdict"].tolist() == [1] and r["n_mps"].tolist() == [11]
    assert r["mp_nobs"].tolist() == [3] * 4 + [2] * 3 + [3] * 3 and (r["mp_flags"] & 1).tolist() == [0] * 4 + [1] * 3 + [0] * 3
    assert r["alive"].reshape(10, 4).tolist() == [[0, 1, 1, 1]] * 4 + [[0] * 4] * 3 + [[0, 1, 1, 1]] * 3


def test_cull_id0():
    c, r = P.case("cull_id0"), _cull("cull_id0")
    assert r["verdict"].tolist() == [3, 1] and r["n_mps"].tolist() == [0, 10] and r["n_redundant"].tolist() == [0, 10]
    assert r["mp_nobs"][:10].tolist() == c["t"]["mp_nobs"][:10].tolist()


def test_mpcull_cases():
    c = P.case("mpcull_cases")
    got = P.expected("mpcull_cases")
    assert np.array_equal(got, c["want"]) and set(got.tolist()) == {0, 1, 2, 3, 4}
    assert (c["mp_visible"] == 0).sum() == 3


def test_random_maps_reach_every_branch():
    sizes = P.RANDOM_SIZES
    assert all(k <= 40 and p <= 2000 and o <= 12 for k, p, o in sizes.values())
    verdicts, cases = set(), set()
    for seed in sizes:
        r = P.expected("random_cull_%d" % seed)
        verdicts |= set(r["verdict"].tolist())
        cases |= set(P.expected("random_mpcull_%d" % seed).tolist())
        v = P.expected("random_vote_%d" % seed, 1)
        assert v["cnt_off"][-1] > 0 and not all(np.array_equal(v[k], P.expected("random_vote_%d" % seed, 0)[k]) for k in P.VOTE_KEYS)
    assert verdicts == {0, 1, 2, 3} and cases == {0, 1, 2, 3, 4}
    big = P.expected("random_cull_0")
    frozen = _cull("random_cull_0", frozen=True)
    assert (big["verdict"] == 1).sum() >= 2 and not np.array_equal(big["verdict"], frozen["verdict"])  # the sequence matters on this map
