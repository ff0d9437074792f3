"""The designed inputs of tests/stereo_search_patterns.py on the CPU: the restatement (tests/stereo_search_restatement.py) must give each case's closed-form result, and every
case's precondition -- that it sits where it says it sits, and that the monocular search the library had answers differently where the stereo branch matters -- is asserted here,
so that tests/test_stereo_search_gpu.py can hold the device to the restatement without skipping or filtering anything."""
import numpy as np
import pytest

from tests import match_patterns as P
from tests import stereo_search_patterns as SP
from tests import stereo_search_restatement as R

f32 = np.float32


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", SP.designed_cases(), ids=_ids(SP.designed_cases()))
def test_restatement_gives_the_closed_form(case):
    tm, n, d, _ = case.restate()
    if case.closed is not None:
        assert np.array_equal(tm, case.closed[0]) and n == case.closed[1]
    if case.want_direction is not None:
        assert d == case.want_direction


def test_directions_reach_all_three_and_sit_on_the_ulp():
    cases = SP.direction_cases()
    assert {c.restate()[2] for c in cases} == {R.NEITHER, R.FORWARD, R.BACKWARD}
    by = {c.name: c for c in cases}
    mb = f32(SP.MB)
    for name, z in (("dir_equal", mb), ("dir_above", P.above(mb)), ("dir_below", P.below(mb)), ("back_equal", -mb), ("back_above", -P.above(mb)), ("back_below", -P.below(mb))):
        got = R.tlc_z(by[name].Tcw, by[name].Tlw)
        assert got.dtype == np.float32 and got == f32(z)  # with Tcw = I the camera centre is -0 and tlc.z is LastFrame's tz to the bit
    assert by["mono_large"].mono == 1 and R.tlc_z(by["mono_large"].Tcw, by["mono_large"].Tlw) > mb and by["mono_large"].restate(mono=0)[2] == R.FORWARD
    for seed in (1, 2, 3, 4):  # the baseline of a general pair is tlc.z's magnitude itself / one ulp below it
        on, under = by["general%d_on" % seed], by["general%d_under" % seed]
        z = abs(R.tlc_z(on.Tcw, on.Tlw))
        assert f32(on.mb) == z and f32(under.mb) == P.below(z) and on.restate()[2] == R.NEITHER and under.restate()[2] != R.NEITHER
    assert {by["general%d_under" % s].restate()[2] for s in (1, 2, 3, 4)} == {R.FORWARD, R.BACKWARD}


@pytest.mark.parametrize("o", [0, 7])
def test_level_ranges_give_three_different_match_vectors(o):
    got = {d: tuple(SP.level_case(o, d).restate()[0]) for d in (R.FORWARD, R.BACKWARD, R.NEITHER)}
    assert len(set(got.values())) == 3
    # the monocular entry (levels o - 1 .. o + 1 whatever the motion) answers a moving stereo pair differently
    for d in (R.FORWARD, R.BACKWARD):
        c = SP.level_case(o, d)
        assert not np.array_equal(c.restate(mono=1)[0], c.restate()[0])
    if o == 0:  # forward with o = 0 checks no level: the level-7 key point is accepted
        c = SP.level_case(0, R.FORWARD)
        assert c.keys["octave"][np.nonzero(c.restate()[0] == 0)[0][0]] == 7


def test_u_right_case_sits_on_the_radius():
    c = SP.u_right_case()
    er = lambda q, t: abs(f32(c.ur[q] - c.u_right[t]))
    assert er(0, 0) == c.radius and er(5, 5) == c.radius                                      # er == radius: kept
    assert er(1, 1) > c.radius and c.u_right[1] == P.above(f32(c.ur[1] + c.radius))            # one ulp of the coordinate outside
    assert er(6, 6) > c.radius and c.u_right[6] == P.below(f32(c.ur[6] - c.radius))
    assert c.u_right[2] == 0.0 and er(2, 2) > c.radius and c.u_right[3] == -1.0               # not tested, although far outside
    assert 0 < c.u_right[4] < 1e-44 and er(4, 4) > c.radius                                    # the smallest positive float is tested
    for q, name in enumerate(SP.UR_SPOTS):
        assert R.drops(c.ur[q], c.u_right[q], c.radius) == (not SP.UR_KEPT[name])
    # winner change: the monocular and the stereo restatement disagree
    mono, stereo = c.restate(stereo_test=False)[0], c.restate()[0]
    assert mono[7] == 7 and mono[8] == -1 and stereo[7] == -1 and stereo[8] == 7
    assert P.hamming(c.qdesc[7], c.desc[7]) < P.hamming(c.qdesc[7], c.desc[8])


def test_u_right_ulp_case_sits_on_the_ulp_of_the_radius():
    c = SP.u_right_ulp_case()
    er = lambda t: abs(f32(c.ur[t] - c.u_right[t]))
    assert all(SP.f32(q[0] - f32(c.bf)) == f32(14.0) for q in c.qxy)
    assert er(0) == c.radius and er(1) == P.above(c.radius)
    assert er(2) == c.radius and float(c.ur[2]) - float(c.u_right[2]) > float(c.radius)  # the exact difference is above the radius, the float is not
    assert [R.drops(c.ur[t], c.u_right[t], c.radius) for t in range(3)] == [False, True, False]


def test_domino_runs_through_the_test():
    c = SP.domino_stereo()
    tm, n, _, _ = c.restate()
    mono = c.restate(stereo_test=False)[0]
    assert R.drops(SP.ur_of(c, 0, 1.0), c.u_right[0], 10.0) and not R.drops(SP.ur_of(c, 1, 2.0), c.u_right[0], 10.0)
    assert abs(f32(SP.ur_of(c, 1, 2.0) - c.u_right[0])) == f32(10.0)
    assert tm[0] == 1 and tm[1] == 0 and mono[0] == 0 and not np.array_equal(mono, tm) and c.blocks[1] == 0 and n == 64
    assert np.array_equal(tm[2:64], np.arange(2, 64))  # every later query still finds its key point claimed and moves on


def test_local_ratio_rule_accepts_what_the_mono_search_rejects():
    c = SP.local_ratio_case()
    tm, n, _, _ = c.restate()
    mono, nmono, _, _ = c.restate(stereo_test=False)
    assert nmono == 0 and (mono < 0).all() and n == 2 and tm[0] == 0 and tm[4] == 2
    assert abs(f32(c.xr[1] - c.u_right[3])) == c.radius and abs(f32(c.xr[2] - c.u_right[5])) > c.radius
    assert (c.keys["octave"] == 0).all() and f32(f32(4.0) * f32(c.th / 4.0)) * c.sf[0] == c.radius


@pytest.mark.parametrize("nq", SP.SEAM_COUNTS)
@pytest.mark.parametrize("kind", ["proj", "local"])
def test_counted_seams(nq, kind):
    c = SP.counted_stereo(nq, kind)
    assert len(c.qxy) == nq and not np.array_equal(c.restate()[0], c.restate(stereo_test=False)[0])
    assert int((c.u_right > 0).sum()) >= nq // 3


@pytest.mark.parametrize("w", SP.WINDOW_SEAMS)
def test_window_seams(w):
    c = SP.window_case(*w)
    assert P.n_cells(w[0], w[1], w[2]) == w[3]
    after, before = c.restate()[3], c.restate(stereo_test=False)[3]
    assert 0 < after < before  # dropped candidates among the kept ones
    assert c.restate()[1] == 1


def test_rs_nc_survivors():
    c = SP.rs_nc_stereo()
    grid = P.grid_lists(c.keys)
    for q, want in enumerate(c.survivors):
        cand = P.area(c.keys, grid, c.qxy[q, 0], c.qxy[q, 1], 10.0, -1, 1)
        kept = [t for t in cand if not R.drops(SP.ur_of(c, q), c.u_right[t], 10.0)]
        assert len(kept) == want and len(cand) > want
        if want:  # dropped ones interleaved: the kept candidates are not a prefix of the list
            assert cand[:want] != kept
    assert not np.array_equal(c.restate()[0], c.restate(stereo_test=False)[0])


@pytest.mark.parametrize("kind", ["proj", "local"])
def test_equivalences_on_the_match_patterns_cases(kind):
    cases = SP.equivalence_cases(kind)
    assert len(cases) >= 15
    for c, S in zip(cases, [S for S in P.claim_cases(P.PROJ if kind == "proj" else P.LOCAL) if len(S.t) <= SP.EQUIVALENCE_MAX_TRAIN]):
        assert not (c.u_right > 0).any()
        tm, n, d, _ = c.restate()
        want, nwant, _ = P.resolve(P.PROJ if kind == "proj" else P.LOCAL, S)
        assert d == R.NEITHER and np.array_equal(tm, want) and n == nwant
        tm1, n1, _, _ = c.restate(mono=1)
        assert np.array_equal(tm1, want) and n1 == nwant
