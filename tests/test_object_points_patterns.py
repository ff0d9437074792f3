"""CPU: every designed input of tests/object_points_patterns.py holds what its name says, judged by the restatement (tests/object_points_restatement.py), and no triangulation
case lies where the reference's float SVD and the stated f64 Jacobi could disagree on a status.

The margin.  A float SVD returns the null vector of A with an error of the order of 2^-24 sigma_1 / sigma_3 (sigma_4 ~ 0 here), so x3D moves by about that times |x3D|;
tests/test_object_points_restatement_pins.py measures at most R.MAX_X3D_UNITS = 3.5 such units between the reference's text and the stated Jacobi on these cases and bounds every
point at R.TOL_X3D = 35.  The cases here are held to MARGIN_UNITS = 1000 units: |w| and |dist - 5| must both exceed 1000 * 2^-24 * sigma_1 / sigma_3 (* |x3D|), well beyond
that bound."""
import numpy as np
import pytest

from tests import object_points_patterns as P
from tests import object_points_restatement as R

MARGIN_UNITS = 1000.0


def test_margin_is_beyond_the_pins_bound():
    assert MARGIN_UNITS > 10 * R.TOL_X3D and R.TOL_X3D == 10 * R.MAX_X3D_UNITS


def test_case_names():
    assert len(P.TRI_NAMES) == 13 and len(P.OD_NAMES) == 11 and len(set(P.NAMES)) == 24
    for n in P.NAMES:
        assert P.case(n)["kind"] == ("tri" if n in P.TRI_NAMES else "od") and globals_doc(n)


def globals_doc(name):
    return getattr(P, name).__doc__


# ---- the triangulation
def test_block_seams_and_empty_pairs():
    assert len(P.case("tri_no_pairs")["first"]) == 1 and len(P.expected("tri_no_pairs")["status"]) == 0
    assert np.diff(P.case("tri_empty_pair_between")["first"]).tolist() == [5, 0, 4]
    for n in (1, 255, 256, 257):
        c = P.case("tri_total_%d" % n)
        assert c["first"][-1] == n and len(c["first"]) == 3 and (P.expected("tri_total_%d" % n)["status"] == R.TRIANGULATED).all()
    assert P.case("tri_total_1")["first"].tolist() == [0, 0, 1]


def test_statuses():
    w = P.expected("tri_statuses")
    assert w["status"].tolist() == [R.NO_OBSERVATION, R.NO_OBSERVATION, R.TRACKLET, R.TRIANGULATED, R.TOO_FAR, R.TRIANGULATED, R.TRIANGULATED]
    c = P.case("tri_statuses")
    assert c["obj_last"][0] < 0 and c["obj_now"][0] >= 2 and c["obj_now"][1] < 0  # rows outside the tables where nothing reads them
    inf = P.infos("tri_statuses")
    assert 4.98 < float(inf[3]["dist"]) < 5.0 < float(inf[4]["dist"]) < 5.02
    for i in (0, 1, 2, 4):
        assert not w["x3D"][i].any() and not w["pos_to_obj"][i].any() and not w["dpoints"][i].any()
    assert w["x3D"][3].all() and np.array_equal(w["dpoints"], w["pos_to_obj"].astype(np.float64))
    off = P.expected("tri_tracklets_off")
    assert off["status"].tolist() == [1, 1, 0, 0, 4, 0, 0]


def test_w_zero():
    w = P.expected("tri_w_zero")
    assert w["status"].tolist() == [R.TRIANGULATED, R.W_ZERO, R.TRIANGULATED]
    c = P.case("tri_w_zero")
    A = np.array(P.infos("tri_w_zero")[1]["A"])
    assert not A[:, 2].any() and np.linalg.matrix_rank(A) == 3 and R.jacobi_vmin4(A.tolist()) == [0.0, 0.0, 1.0, 0.0]
    assert c["kp1"][1].tolist() == c["kp2"][1].tolist() == [P.K4[2], P.K4[3]]
    # equal poses and equal rays, the first candidate: rank 2, and the w that comes out is tiny but not 0
    A2, v = P.w_zero_candidate()
    assert np.linalg.matrix_rank(np.array(A2), tol=1e-6) == 2 and 0 < abs(v[3]) < 1e-12 and np.float32(v[3]) != 0


def test_motions_and_sources():
    c = P.case("tri_identity_motion")
    assert np.array_equal(c["cub_pose_last"], c["cub_pose_now"]) and not np.array_equal(c["Tcw_last"], c["Tcw_now"])
    Td = R.object_camera(c["Tcw_now"][0], c["cub_pose_now"][0], c["cub_pose_last"][0])
    assert np.abs(np.array(Td, np.float64) - c["Tcw_now"][0]).max() < 1e-6
    c = P.case("tri_static_camera")
    assert np.array_equal(c["Tcw_last"], c["Tcw_now"]) and np.array_equal(c["cub_pose_last"][0, 3:], c["cub_pose_now"][0, 3:]) and not np.array_equal(c["cub_pose_last"], c["cub_pose_now"])
    h, o = P.case("tri_harris_source"), P.case("tri_orb_source")
    assert np.array_equal(o["kp1"], np.round(o["kp1"])) and np.array_equal(o["kp2"], np.round(o["kp2"])) and not np.array_equal(h["kp1"], np.round(h["kp1"]))
    for n in ("tri_identity_motion", "tri_static_camera", "tri_harris_source", "tri_orb_source"):
        w = P.expected(n)
        assert (w["status"] == 0).all()
        # the triangulated point is the point's position at the last key frame: world_pos is 0.1 away by construction (whole pixels move it by centimetres)
        assert np.abs(np.linalg.norm(w["x3D"].astype(np.float64) - P.case(n)["world_pos"], axis=1) - 0.0990).max() < (0.06 if n == "tri_orb_source" else 1e-4)


@pytest.mark.parametrize("name", P.TRI_NAMES)
def test_no_point_near_a_status_change(name):
    """The condition on the triangulation cases: every point that reaches the SVD is MARGIN_UNITS units away from w == 0 and from the distance 5 (the exact zero of tri_w_zero
    excepted, which is exact on both sides: see the patterns module)."""
    for i, info in enumerate(P.infos(name)):
        if "A" not in info:
            continue
        A = np.array(info["A"])
        s = np.linalg.svd(A, compute_uv=False)
        v = R.jacobi_vmin4(info["A"])
        if not A[:, 2].any():
            assert name == "tri_w_zero" and v == [0.0, 0.0, 1.0, 0.0]
            continue
        assert s[2] > 0 and s[0] / s[2] < 10 and s[3] < 1e-2 * s[2], (name, i, s)
        unit = 2.0 ** -24 * s[0] / s[2]
        x = np.array(info["x3D"], np.float64)
        assert abs(v[3]) > MARGIN_UNITS * unit, (name, i)
        assert abs(float(info["dist"]) - 5.0) > MARGIN_UNITS * unit * np.linalg.norm(x), (name, i, float(info["dist"]))


# ---- the object-depth initialisation
def _od(name, mode):
    return P.expected(name, mode)


def test_two_in_cell():
    assert _od("od_two_in_cell", R.TRACKING)["candidates"].tolist() == [0, 2, 4]
    assert _od("od_two_in_cell", R.LOCAL_MAPPING)["candidates"].tolist() == [0, 1, 2, 3, 4] == _od("od_two_in_cell", R.FIRST_FRAME)["candidates"].tolist()
    c = P.case("od_two_in_cell")
    cells = [R.pos_in_grid(k["x"], k["y"], P.BOUNDS)[1:] for k in c["keys"][:4]]
    assert cells[0] == cells[1] == (10, 10) and cells[2] == cells[3] == (23, 8)


def test_earlier_nonqualifying():
    t = _od("od_earlier_nonqualifying", R.TRACKING)
    assert t["candidates"].tolist() == [2, 3, 5] and t["raw_depth_pts"].tolist() == [1]
    assert _od("od_earlier_nonqualifying", R.LOCAL_MAPPING)["candidates"].tolist() == [0, 2, 3, 5]  # no octave test there
    c = P.case("od_earlier_nonqualifying")
    cell = lambda i: R.pos_in_grid(c["keys"]["x"][i], c["keys"]["y"][i], P.BOUNDS)[1:]
    assert cell(0) == cell(2) and cell(1) == cell(3) and cell(4) == cell(5) and c["keys"]["octave"][0] == 3 and c["object_id"][1] == -1 and c["has_map_point"][4]


def test_outside_grid():
    c = P.case("od_outside_grid")
    inside = [R.pos_in_grid(k["x"], k["y"], P.BOUNDS) for k in c["keys"][:7]]
    assert [i[0] for i in inside] == [False, True, False, False, True, True, False]
    assert inside[1][1] == 63 and inside[2][1] == 64 and inside[3][2] == 48 and inside[4][2] == 47 and inside[5][1] == 0 and inside[6][1] == -1
    assert _od("od_outside_grid", R.TRACKING)["candidates"].tolist() == [1, 4, 5]
    assert _od("od_outside_grid", R.LOCAL_MAPPING)["candidates"].tolist() == list(range(7))


def test_truncated_bounds():
    c = P.case("od_truncated_bounds")
    cells = [R.pos_in_grid(k["x"], k["y"], P.UNDISTORTED_BOUNDS)[1:] for k in c["keys"][:4]]
    assert cells[0] == (10, 20) and cells[1] == (11, 20) and cells[2][1] == 10 and cells[3][1] == 11 and cells[2][0] == cells[3][0]
    assert _od("od_truncated_bounds", R.TRACKING)["candidates"].tolist() == [0, 1, 2, 3]
    # with Frame's float mnMinX / mnMinY the two pairs would share a cell each
    F = np.float32
    w, h = F(64) / F(F(643.5) - F(-3.7)), F(48) / F(F(482.3) - F(-2.6))
    assert [round(float((F(x) - F(-3.7)) * w)) for x in (102.875, 108.0)] == [11, 11] and [round(float((F(y) - F(-2.6)) * h)) for y in (103.567, 108.5)] == [11, 11]


def test_ratio_turn():
    assert 3.0 / 10.0 == 0.30 and 6.0 / 20.0 == 0.30 and not 3.0 / 10.0 < 0.30
    for mode in (R.TRACKING, R.LOCAL_MAPPING):
        w = _od("od_ratio_turn", mode)
        assert w["raw_depth_pts"].tolist() == [3, 2, 6, 5, 2] and w["max_initialize_pts"].tolist() == [-1, 1, -1, 1, 0] and np.diff(w["new_first"]).tolist() == [0, 1, 0, 1, 0]
    assert P.off_integer_totals() == [] and int(9 * 0.30) == 2 and int(30 * 0.30) == 9


def test_more_than_80_and_max_zero():
    t, l = _od("od_more_than_80", R.TRACKING), _od("od_more_than_80", R.LOCAL_MAPPING)
    assert t["n_candidates"].tolist() == [100] == l["n_candidates"].tolist() and t["max_initialize_pts"].tolist() == [80] and l["max_initialize_pts"].tolist() == [100]
    assert len(t["new_idx"]) == 80 and len(l["new_idx"]) == 100 and sorted(l["shuffled"].tolist()) == l["candidates"].tolist() and l["shuffled"].tolist() != l["candidates"].tolist()
    assert np.array_equal(t["shuffled"][:80], l["shuffled"][:80])  # the same draws
    z = _od("od_max_zero", R.TRACKING)
    assert z["n_candidates"].tolist() == [3] and z["max_initialize_pts"].tolist() == [0] and len(z["new_idx"]) == 0 and z["shuffled"].tolist() == [0, 1, 2]


def test_walk_past_and_depths():
    for mode in (R.TRACKING, R.LOCAL_MAPPING):
        w = _od("od_walk_past", mode)
        assert w["max_initialize_pts"].tolist() == [9] and w["shuffled"][:4].tolist() == [0, 1, 2, 3] and len(w["new_idx"]) == 8
        assert w["new_idx"].tolist() == w["shuffled"][4:].tolist() and set(w["shuffled"][9:].tolist()) & set(w["new_idx"].tolist())  # entries behind max_initialize_pts became points
        d = _od("od_depth_zero", mode)
        assert (P.case("od_depth_zero")["object_id"][d["new_idx"]] == 1).all() and len(d["new_idx"]) == 4 and d["max_initialize_pts"].tolist() == [6]
    assert len(_od("od_depth_zero", R.FIRST_FRAME)["new_idx"]) == 4


def test_same_slot_twice():
    w = _od("od_same_slot_twice", R.TRACKING)
    assert w["candidates"].tolist() == list(range(8)) and w["shuffled"].tolist() == [5, 0, 1, 3, 4, 6, 7, 2]
    assert P.case("od_same_slot_twice")["draws"].tolist() == [5, 4, 3, 0, 0, 7, 7, 7] and w["new_idx"].tolist() == w["shuffled"].tolist()


def test_batch_and_modes():
    c = P.case("od_batch")
    assert np.diff(c["first"]).tolist() == [17, 25, 20, 0, 24, 400, 30]
    for mode in P.MODES:
        w = _od("od_batch", mode)
        assert w["n_candidates"][1] == 0 and w["n_candidates"][3] == 0 and w["cand_first"][-1] == len(w["candidates"]) and w["new_first"][-1] == len(w["new_idx"])
        # every frame of the batch is the single-frame case's answer
        for f, name in ((0, "od_two_in_cell"), (2, "od_earlier_nonqualifying"), (4, "od_outside_grid"), (5, "od_more_than_80"), (6, "od_walk_past")):
            one = _od(name, mode)
            assert w["new_idx"][w["new_first"][f]:w["new_first"][f + 1]].tolist() == one["new_idx"].tolist()
            assert w["new_x3D"][w["new_first"][f]:w["new_first"][f + 1]].tobytes() == one["new_x3D"].tobytes()
    assert _od("od_batch", R.TRACKING)["max_initialize_pts"][3] == -1  # no key points: 0 / 0 is not below 0.30
    names = {m: _od("od_batch", m)["new_idx"].tolist() for m in P.MODES}
    assert len({str(v) for v in names.values()}) == 3  # the three modes differ on the same table


def test_unprojection_uses_the_frames_pose():
    w = _od("od_two_in_cell", R.FIRST_FRAME)
    c = P.case("od_two_in_cell")
    T = c["Twc"][0].astype(np.float64).reshape(3, 4)
    for j, i in enumerate(w["new_idx"]):
        z = float(c["cuboid_depth"][c["object_id"][i]])
        xc = np.array([(c["keys"]["x"][i] - P.K4[2]) * z / P.K4[0], (c["keys"]["y"][i] - P.K4[3]) * z / P.K4[1], z])
        assert np.abs(T[:, :3] @ xc + T[:, 3] - w["new_x3D"][j]).max() < 1e-5
