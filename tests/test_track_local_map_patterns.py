"""CPU: the inputs of the TrackLocalMap GPU tests take every path they are meant to take, checked with the restatement alone (tests/track_local_map_restatement.py): every
reject class of Frame::isInFrustum, both radius classes, contested key points at the widest th, the constructed exact cases (a point ON every bound, float(0.998) against the
double 0.998, the ends of the scale table, PcZ == 0), and the key-frame graphs (a parent push that ends the expansion, the 80-frame stop, a tie for pKFmax).  The host walk of the
library (cs_track_local_keyframes) is held to the restatement here as well: it needs no device."""
import numpy as np
import pytest

from tests import sim3_restatement as S
from tests import track_local_map_restatement as R

@pytest.fixture(scope="module")
def frames(oracle):
    return S.frames(oracle)


@pytest.fixture(scope="module")
def case(oracle, frames):
    T, pts, blocks, tb = R.local_points(frames, 700)
    fr = R.frustum_all(pts, *T, R.INTR, R.BOUNDS, R.LOG_SF, len(R.SF))
    return T, pts, blocks, tb, fr, S.make_frame(oracle, *frames[0])


def test_reject_classes(case):
    T, pts, blocks, tb, fr, F = case
    for c in R.REJECTS:
        assert sum(1 for r in fr["reason"] if r == c) >= 10, c
    assert 0 < fr["in_view"][:255].sum() < 255  # (the small sizes of the GPU tests are mixed too)
    assert fr["in_view"].sum() >= 1500 and len(pts["skip"]) == 3000


@pytest.mark.parametrize("th", [1.0, 3.0, 5.0])
def test_radius_classes_and_contested(oracle, case, th):
    T, pts, blocks, tb, fr, F = case
    st = {}
    out = R.search_local_points(oracle, F, *T, pts, blocks, R.INTR, R.BOUNDS, R.LOG_SF, R.SF, th, 0.8, tb, stats=st, fr=fr)
    assert st["radius"][2.5] >= 10 and st["radius"][4.0] >= 10, st["radius"]
    assert out["nmatches"] >= 100 and not np.any(out["train_match"][tb != 0] >= 0)
    if th == 5.0:
        assert st["contested"] >= 20, st
    assert out["nmatches"] >= int((out["train_match"] >= 0).sum())  # (an assignment that a later point overwrote is counted too)
    # the search half alone against the oracle's SearchByProjection(F, vpMapPoints, th), which is pinned to the reference elsewhere
    tm, nm = oracle.search_local_map(F[2], fr["proj"][:, :2], fr["view_cos"], np.maximum(fr["pred_level"], 0), fr["in_view"], blocks, pts["mp_desc"], R.SF, th, 0.8, tb)
    assert nm == out["nmatches"] and np.array_equal(tm, out["train_match"])


def test_exact_cases():
    f32 = np.float32
    assert f32(f32(0.8) * f32(5.0)) == f32(4.0) and float(f32(0.998)) > 0.998 and not (f32(0.998) > f32(0.998))
    for name, log_sf, sf, pts, want in R.exact_cases():
        fr = R.frustum_all(pts, *R.EX_POSE, R.EX_INTR, R.EX_BOUNDS, log_sf, len(sf))
        for i, (iv, lvl, rad) in enumerate(want):
            assert fr["in_view"][i] == iv, (name, i, fr["reason"][i])
            if iv:
                assert fr["pred_level"][i] == lvl and float(R.radius_by_viewing_cos(fr["view_cos"][i])) == rad, (name, i, fr["pred_level"][i], fr["view_cos"][i])
        if name == "sf2":
            assert tuple(fr["proj"][0][:2]) == (0.0, 240.0) and tuple(fr["proj"][1][:2]) == (640.0, 240.0) and fr["proj"][2][1] == 0.0 and fr["proj"][3][1] == 480.0
            assert fr["view_cos"][6] == f32(0.5) and fr["view_cos"][7] == f32(0.998)
            assert fr["reason"][11] == "outside" and fr["reason"][12] == "image" and fr["reason"][13] == "depth" and fr["reason"][14] == "image"
            assert fr["proj"][0][2] == f32(0.0 - 40.0)  # uR = u - bf * invz
        else:
            assert fr["reason"][0] == "outside" and fr["reason"][3] == "outside"


def _walk(g):
    from cube_slam_amd.tracking import track_local_keyframes
    return track_local_keyframes(g["frame_mp"], g["mp_skip"], g["obs_off"], g["obs_kf"], g["kf_bad"], g["cov_off"], g["cov_kf"], g["child_off"], g["child_kf"], g["parent"])


def test_keyframe_graphs_take_their_paths():
    g = R.graph_case("parent_break")
    loc, mx = R.update_local_keyframes(**g)
    assert loc.tolist() == [2, 5, 7, 3, 4, 0] and mx == 2  # 5's neighbour 8 and 7's neighbour 9 are never reached; the tie 2 / 5 goes to the first
    g = R.graph_case("stop_80")
    loc, mx = R.update_local_keyframes(**g)
    assert len(loc) == 81 and loc[:79].tolist() == list(range(79)) and loc[79:].tolist() == [100, 101]
    g = R.graph_case("tie_max")
    loc, mx = R.update_local_keyframes(**g)
    assert mx == 3 and loc.tolist() == [3, 4, 6]
    g = R.graph_case("bad_and_none")
    loc, mx = R.update_local_keyframes(**g)
    assert mx == 4 and loc.tolist() == [1, 4, 10, 12] and 11 not in loc  # 2 has the most votes and is bad: pKFmax is 4
    assert R.update_local_keyframes(**R.graph_case("no_votes")) == (None, -1)
    loc, mx = R.update_local_keyframes(**R.graph_case("random"))
    assert len(loc) > 20 and len(set(loc.tolist())) == len(loc)


@pytest.mark.parametrize("name", R.GRAPHS)
def test_library_walk_equals_restatement(name):
    g = R.graph_case(name)
    want, wmx = R.update_local_keyframes(**g)
    got, gmx = _walk(g)
    assert gmx == wmx and (got is None) == (want is None) and (want is None or np.array_equal(got, want))


def test_library_walk_rejects_bad_indices():
    from cube_slam_amd._lib import CubeSlamError
    g = R.graph_case("tie_max")
    g["obs_kf"] = g["obs_kf"].copy(); g["obs_kf"][0] = 99
    with pytest.raises(CubeSlamError, match="CS_ERR_BAD_ARG"):
        _walk(g)


def test_update_local_points_lists():
    off, mp = R.keyframe_lists(5, 40, 30, 3)
    skip = (np.arange(40) % 7 == 0).astype(np.uint8)
    out = R.update_local_points(off, mp, skip)
    assert len(set(out.tolist())) == len(out) and not np.any(skip[out]) and set(out.tolist()) == {int(x) for x in mp if x >= 0 and not skip[x]}
    first = {int(x): i for i, x in reversed(list(enumerate(mp))) if x >= 0}
    assert [first[int(x)] for x in out] == sorted(first[int(x)] for x in out)
