"""Preconditions of the PoseOptimization edge tests, checked on the CPU from the oracle alone (tests/pose_patterns.py, orc_pose_optimization_trace): a case that claims a path
of Optimizer::PoseOptimization must take it, equal flags are a fair demand only where no chi2 sits on its threshold, and a tolerance derived from round-off only where no
decision of the run flips when the edges are merely reordered."""
import numpy as np
import pytest

from tests import pose_patterns as P


@pytest.mark.parametrize("name", list(P.CASES))
def test_case_takes_the_path_it_claims(oracle, name):
    fr = P.case(name)
    pose, flags, n_in, tr = P.judged(oracle, name)
    claims = P.CASES[name][1]
    n = len(flags)
    assert claims and n == P.CASES[name][0]["n"] and np.all(np.isfinite(pose)) and n_in == (n - int(flags.sum()) if n >= 3 else 0)
    for k in ("active", "iterations", "trials", "rejected", "failed_solves", "exits"):
        assert len(tr[k]) == tr["rounds"]
    assert tr["iterations_total"] == sum(tr["iterations"]) and tr["trials_total"] == sum(tr["trials"]) >= tr["iterations_total"]
    assert tr["rejected_total"] == sum(tr["rejected"]) >= tr["failed_solves_total"] == sum(tr["failed_solves"])
    assert all(1 <= i <= 10 and i <= t <= 10 * i for i, t in zip(tr["iterations"], tr["trials"])) and (tr["rounds"] == 0 or tr["active"][0] == n)
    stays = pose.tobytes() == P.normalised(fr["pose"]).tobytes()
    for claim in claims:
        if claim == "untouched":
            assert n < 3 and tr["rounds"] == 0 and n_in == 0 and not flags.any()
        elif claim == "one_round":
            assert 3 <= n < 10 and tr["rounds"] == 1
        elif claim == "four_rounds":
            assert n >= 10 and tr["rounds"] == 4
        elif claim in ("exit_qmax", "exit_rho0", "exit_nbad", "exit_iterations"):
            assert claim[5:] in tr["exits"]
            if claim == "exit_iterations":
                assert 10 in tr["iterations"]
        elif claim == "rejected":
            assert tr["rejected_total"] > tr["failed_solves_total"]
        elif claim == "failed_solve":
            assert tr["failed_solves_total"] > 0
        elif claim == "failed_every_round":
            assert tr["failed_solves"] == [10, 10, 10, 10] and tr["iterations"] == [1, 1, 1, 1] and tr["exits"] == ["qmax"] * 4
        elif claim == "empty_round":
            assert tr["active"][1] == 0 and tr["failed_solves"][1] == 10  # H = 0, lambda = 0: no solve can succeed
        elif claim == "none_flagged":
            assert not flags.any() and n_in == n
        elif claim == "all_flagged":
            assert flags.all() and n_in == 0
        elif claim == "stays":
            assert stays
        elif claim == "behind":
            assert tr["nonpositive_depth"]
        elif claim == "flips_quat":
            assert fr["pose"][6] < 0 and abs(np.linalg.norm(fr["pose"][3:]) - 2.5) < 1e-12 and abs(np.linalg.norm(pose[3:]) - 1) < 1e-15 and pose[6] > 0
        else:
            raise AssertionError(claim)
    if "stays" not in claims:
        assert not stays
    if "behind" not in claims:
        assert not tr["nonpositive_depth"]


def test_the_set_covers_every_path(oracle):
    tr = {name: P.judged(oracle, name)[3] for name in P.CASES}
    exits = {e for t in tr.values() for e in t["exits"]}
    assert exits == {"qmax", "rho0", "nbad", "iterations"}  # each way out of OptimizationAlgorithmLevenberg::solve
    assert any(t["failed_solves_total"] > 0 for t in tr.values())
    assert any(t["rounds"] == 4 and 0 in t["active"] for t in tr.values())  # a round without an active edge
    assert any(t["rejected_total"] > t["failed_solves_total"] for t in tr.values())  # a trial undone although its solve succeeded
    assert {t["rounds"] for t in tr.values()} == {0, 1, 4}  # n < 3, the single round of n < 10, four rounds
    assert any(t["nonpositive_depth"] for t in tr.values())
    assert any(t["rounds"] == 4 and len(set(t["active"])) > 1 for t in tr.values())  # the active set changes between rounds
    sizes = {P.CASES[name][0]["n"] for name in P.CASES}
    assert set(P.SIZES) <= sizes and {0, 2} <= sizes
    assert {3, 4, 9, 10, 11, 63, 64, 65, P.THREADS - 1, P.THREADS, P.THREADS + 1, 2 * P.THREADS - 1, 2 * P.THREADS, 2 * P.THREADS + 1, 8 * P.THREADS + 1} == set(P.SIZES)


def test_the_cases_are_what_they_are_named():
    for name, (kw, _) in P.CASES.items():
        fr = P.case(name)
        n = kw["n"]
        assert fr["Xw"].shape == (n, 3) and fr["obs"].shape == (n, 3) and fr["inv_sigma2"].shape == (n,) and fr["pose"].shape == (7,) and fr["intr"].shape == (5,)
        for k in ("Xw", "obs", "inv_sigma2"):  # what the reference reads out of float Mats and float key points
            assert np.array_equal(fr[k], fr[k].astype(np.float32).astype(np.float64)) and np.all(np.isfinite(fr[k])), (name, k)
        assert np.array_equal(fr["obs"][:, 2] >= 0, fr["is_stereo"]) and np.all(fr["obs"][~fr["is_stereo"], 2] == -1.0)
    for n in P.SIZES:  # about 20 % gross outliers, each moved by 15 px or more
        kw = P.CASES["n%d" % n][0]
        fr = P.case("n%d" % n)
        clean = P.make_frame(**dict(kw, outliers=0.0))
        k = int(fr["is_outlier"].sum())
        assert k == int(round(0.2 * n)) and k >= 1
        moved = np.abs(fr["obs"][:, :2] - clean["obs"][:, :2])
        assert np.all(moved[fr["is_outlier"]] >= 14.99) and np.all(moved[~fr["is_outlier"]] == 0)
    for triple in ((3, 4), (9, 10, 11), (63, 64, 65), (255, 256, 257), (511, 512, 513)):  # of every seam triple one mixed and one all stereo
        share = [P.case("n%d" % n)["is_stereo"].mean() for n in triple]
        assert any(0 < s < 1 for s in share) and any(s == 1 for s in share), triple
    assert 0 < P.case("n2049")["is_stereo"].mean() < 1
    fr = P.case("all_outliers")
    assert fr["is_outlier"].all() and np.all(np.abs(fr["obs"][:, :2] - P.make_frame(**dict(P.CASES["all_outliers"][0], outliers=0.0))["obs"][:, :2]) >= 14.99)
    assert not P.case("zero_weights")["inv_sigma2"].any()
    fr = P.case("far_start")
    assert np.linalg.norm(fr["pose"][:3] - fr["pose_true"][:3]) > 7.99 and np.array_equal(fr["pose"][3:], fr["pose_true"][3:])
    assert np.array_equal(P.case("exact_start")["pose"], P.case("exact_start")["pose_true"])
    fr = P.case("behind_camera")
    assert fr["mirrored"].sum() == 20 and np.array_equal(fr["Xw"][fr["mirrored"]], -P.make_frame(**dict(P.CASES["behind_camera"][0], mirror=0.0))["Xw"][fr["mirrored"]])
    fr = P.case("one_point")
    assert len(fr["Xw"]) == 20 and np.all(fr["Xw"] == fr["Xw"][0]) and np.all(fr["obs"] == fr["obs"][0]) and np.all(fr["inv_sigma2"] == fr["inv_sigma2"][0])
    a, b = P.case("cam_kitti"), P.case("cam_tum")  # one geometry, two cameras
    assert np.array_equal(a["Xw"], b["Xw"]) and np.array_equal(a["pose"], b["pose"]) and np.array_equal(a["inv_sigma2"], b["inv_sigma2"])
    assert np.array_equal(a["is_stereo"], b["is_stereo"]) and np.array_equal(a["is_outlier"], b["is_outlier"]) and np.all(np.abs(a["intr"] - b["intr"]) > 50)
    a, b = P.case("bf_a"), P.case("bf_b")  # one stereo frame, two rigs
    for k in ("Xw", "obs", "inv_sigma2", "pose"):
        assert np.array_equal(a[k], b[k])
    assert a["is_stereo"].all() and np.array_equal(a["intr"][:4], b["intr"][:4]) and a["intr"][4] != b["intr"][4]


def test_the_batch_is_what_the_device_test_needs():
    n = [P.CASES[k][0]["n"] for k in P.BATCH]
    off = np.cumsum(n)
    assert len(P.BATCH) >= 8 and len(set(P.BATCH)) == len(P.BATCH) and np.all(off % 2 == 1)  # every edge offset after the first is odd
    i0, i2 = n.index(0), n.index(2)
    assert min(n[i0 - 1], n[i0 + 1], n[i2 - 1], n[i2 + 1]) >= 256 and i0 > 0 and i2 > 0
    cams = [tuple(P.case(k)["intr"]) for k in P.BATCH]
    assert sum(a != b for a, b in zip(cams, cams[1:])) >= 4 and len(set(cams)) == 3


@pytest.mark.parametrize("name", list(P.CASES))
def test_no_chi2_sits_on_its_threshold(oracle, name):
    assert P.judged(oracle, name)[3]["min_margin"] >= P.MARGIN


@pytest.mark.parametrize("name", list(P.CASES))
def test_order_sensitivity(oracle, name):
    """The oracle under four permutations of a case's edges: the same flags and count, and a pose within D_REF_FIT (no decision flipped) and within the recorded D_REF."""
    d, same_flags, same_count = P.order_sensitivity(oracle, name)
    print("%s: d_ref %.3e (D_REF %.3e)" % (name, d, P.D_REF))
    assert same_flags and same_count
    assert d <= P.D_REF_FIT
    assert d <= P.D_REF


def test_the_tolerance_is_tighter_than_the_old_one(oracle):
    assert P.D_REF == max(P.order_sensitivity(oracle, name)[0] for name in P.CASES)
    assert P.TOL == 100 * P.D_REF and 0 < P.TOL < 1e-8


def test_the_unfit_kind_exists(oracle):
    """What D_REF_FIT sorts out: a frame of tests/test_pose_gpu.py in which a decision flips under reordering, so that the oracle lands a thousand times further away than
    in any case here."""
    from cube_slam_amd import synth
    fr = synth.pose_frame(10, n=800, outlier_frac=0.15)
    pose = P.run(oracle, fr)[0]
    d = max(P.pose_distance(P.run(oracle, fr, np.random.default_rng(s).permutation(800))[0], pose) for s in P.PERMUTATION_SEEDS)
    assert d > 100 * P.D_REF_FIT
