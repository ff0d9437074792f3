"""Preconditions of the Sim3 refinement's tests, checked on the CPU from the restatement alone (tests/sim3_opt_restatement.py): exact equality of flags and counts is a
fair demand only where no chi2 at a cut sits on the threshold, and a case that claims a path of Optimizer::OptimizeSim3 must take it."""
import numpy as np
import pytest

from tests import sim3_opt_restatement as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_no_chi2_sits_on_the_threshold(name):
    _, _, _, st = R.judged(name)
    assert st["margin"] > 1e-3


@pytest.mark.parametrize("name", list(R.CASES))
def test_case_takes_the_path_it_claims(name):
    c = R.case(name)
    pose, removed, n_in, st = R.judged(name)
    claims = R.CASES[name][1]
    assert claims
    n = len(removed)
    for claim in claims:
        if claim == "early":
            assert st["early"] and not st["stage2"] and n_in == 0 and n - st["nbad1"] < 10 and pose.tobytes() == np.ascontiguousarray(c["sim3_in"], np.float64).tobytes()
        elif claim == "stage2":
            assert st["stage2"] and not st["early"] and n_in == n - st["nbad1"] - st["nbad2"] and n_in >= 10 - st["nbad2"]
        elif claim == "nbad0":
            assert st["nbad1"] == 0
        elif claim == "nbad>0":
            assert st["nbad1"] > 0
        elif claim == "nbad2>0":
            assert st["nbad2"] > 0
        elif claim == "outliers_exact":
            assert len(c["outliers"]) == 3 and np.array_equal(np.nonzero(removed)[0], c["outliers"])
        elif claim.startswith("exits:"):
            want = claim[6:].split(",")
            assert len(st["exits"]) == len(want) and all(w in ("*", e) for w, e in zip(want, st["exits"])) and set(st["exits"]) <= set(R.EXITS)
        elif claim == "failed_solves":  # every trial of both stages: ten per iteration, lambda stays 0
            assert st["failed_solves"] == len(st["trace"]) == 20 and not st["trace"][:, 5].any() and not st["trace"][:, 6].any() and not st["trace"][:, 4].any()
            assert not st["system0"].any() and not st["branches"]
        elif claim == "pose_unmoved":
            assert st["stage2"] and pose.tobytes() == np.ascontiguousarray(c["sim3_in"], np.float64).tobytes()
        elif claim == "all_inliers":
            assert n_in == n and not removed.any()
        elif claim == "all_flagged":
            assert removed.all() and st["nbad1"] == n
        elif claim == "ten_left":
            assert n - st["nbad1"] == 10 and n_in == 10 - st["nbad2"]
        elif claim == "behind_flagged":
            i = R.CASES[name][0]["behind"][0]
            assert c["P2c"][i, 2] < 0 and (np.delete(c["P2c"][:, 2], i) > 0).all() and removed[i] == 1 and np.isfinite(pose).all() and np.isfinite(st["trace"]).all()
        elif claim == "scale_kept":
            assert c["fix_scale"] and pose[7] == c["sim3_in"][7] and pose.tobytes() != np.ascontiguousarray(c["sim3_in"], np.float64).tobytes()
        elif claim == "stage2_its>=6":
            assert st["stage_iterations"][1] >= 6
        elif claim == "stage2_its==5":
            assert st["stage_iterations"][1] == 5
        elif claim == "budget_matters":  # a kernel that always gave stage two 5 iterations, or always 10, fails this case
            other = R.optimize_sim3(c, stage2_budget=5 if st["nbad1"] > 0 else 10)
            assert R.pose_distance(other[0], pose) > 100 * R.TOL or not np.array_equal(other[1], removed)
        else:
            raise AssertionError(claim)
    assert int(removed.sum()) == st["nbad1"] + st["nbad2"]


def test_the_set_covers_every_path():
    st = {name: R.judged(name)[3] for name in R.CASES}
    assert any(s["rejected"] > 0 for s in st.values())  # a rejected LM trial
    assert any(s["nbad2"] > 0 for s in st.values())  # stage 2 flags a pair
    assert any(s["stage2"] and s["nbad1"] == 0 for s in st.values()) and any(s["stage2"] and s["nbad1"] > 0 for s in st.values())  # 5 and 10 more iterations
    assert any(s["early"] and s["nbad1"] > 0 for s in st.values())  # the early return keeps its flags
    sizes = {len(R.judged(name)[1]) for name in R.CASES}
    assert {0, 9, 10, 11, 12, R.THREADS - 1, R.THREADS, R.THREADS + 1, 2000} <= sizes


def test_the_cases_are_what_the_issue_asks():
    for name, (kw, _) in R.CASES.items():
        c = R.case(name)
        n = kw["n"]
        assert c["P1c"].shape == (n, 3) and c["P2c"].shape == (n, 3)
        if n:
            z2 = c["P2c"][:, 2].copy()
            z2[list(kw.get("behind", ()))] *= -1  # a point mirrored behind the camera on purpose is as deep as it was
            assert 2.0 <= c["P1c"][:, 2].min() and c["P1c"][:, 2].max() <= 20.0 and 2.0 <= z2.min() and z2.max() <= 20.0
            for k in ("P1c", "P2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "intrinsics"):  # what the reference holds in floats
                assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k
        if not kw.get("same_k"):
            assert not np.array_equal(c["intrinsics"][:4], c["intrinsics"][4:])
        clean = R.make_case(**dict(kw, n_outliers=0, moved=())) if len(c["outliers"]) else None
        for i in c["outliers"]:
            assert max(np.linalg.norm(c["obs1"][i] - clean["obs1"][i]), np.linalg.norm(c["obs2"][i] - clean["obs2"][i])) >= 29.9
    assert [R.CASES[k][0]["s"] for k in ("scale_0.5", "scale_1", "scale_2")] == [0.5, 1.0, 2.0]
    batch_n = [R.CASES[k][0]["n"] for k in R.BATCH]
    assert len(R.BATCH) == 7 and len(set(batch_n)) == 7 and 0 in batch_n and any(R.judged(k)[3]["early"] and R.CASES[k][0]["n"] > 0 for k in R.BATCH)
    assert R.CASES["fix_scale_on"][0]["fix_scale"] and R.judged("fix_scale_on")[0][7] == R.case("fix_scale_on")["sim3_in"][7]
    assert R.judged("fix_scale_off")[0][7] != R.case("fix_scale_off")["sim3_in"][7]


# ------------------------------------------------------------------------------------------------------------------ the designed cases and the way the optimiser takes
def test_the_set_covers_every_exit_branch_and_a_failed_solve():
    st = {name: R.judged(name)[3] for name in R.CASES}
    assert {e for s in st.values() for e in s["exits"]} == set(R.EXITS)
    assert {b for s in st.values() for b in s["branches"]} == set(R.EXP_BRANCHES)
    for b in R.EXP_BRANCHES:  # each branch by a solved step of a new case, not by luck of the seeded ones
        assert any(b in st[k]["branches"] for k in R.NEW_CASES), b
    assert any(s["failed_solves"] > 0 for s in st.values())
    assert any(s["stage2"] and s["stage_iterations"][1] >= 6 for s in st.values()) and max(len(s["trace"]) for s in st.values()) <= R.MAX_TRIALS
    assert all(R.CASES[k][0]["n"] <= 300 for k in R.NEW_CASES)
    for name, s in st.items():
        assert s["trace"].shape == (s["rejected"] + int(s["trace"][:, 6].sum()), R.TRACE_RECORD) and s["system0"].shape == (36,)
        assert sum(s["stage_iterations"]) == s["iterations"] and len(s["exits"]) == (0 if name == "n0" else 2 if s["stage2"] else 1)


def test_the_pairs_differ_in_one_parameter_and_in_their_results():
    same = lambda a, b, skip: all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a if k not in skip)
    a, b, c = (R.case(k) for k in ("th2_5.991", "th2_7.815", "th2_20"))
    assert same(a, b, ("th2",)) and same(a, c, ("th2",)) and [float(x["th2"]) for x in (a, b, c)] == [float(np.float32(v)) for v in (5.991, 7.815, 20.0)]
    ra, rb, rc = (R.judged(k)[1] for k in ("th2_5.991", "th2_7.815", "th2_20"))
    assert not np.array_equal(ra, rb) and not np.array_equal(rb, rc) and not np.array_equal(ra, rc)
    for k, want in (("th2_5.991", -1), ("th2_7.815", 1), ("th2_20", 0)):  # the Huber threshold (float) (delta * delta) against th2: a last float bit below, above, equal
        P = R._Problem(R.case(k))
        assert np.sign(P.dsqr - P.th2) == want and abs(P.dsqr - P.th2) <= 4.8e-7
    a, b = R.case("k_a"), R.case("k_b")
    assert same(a, b, ("intrinsics",)) and np.array_equal(a["intrinsics"][:4], b["intrinsics"][:4]) and not (a["intrinsics"][4:] == b["intrinsics"][4:]).any()
    assert R.pose_distance(R.judged("k_a")[0], R.judged("k_b")[0]) > 1000 * R.TOL
    a, b = R.case("fix_a"), R.case("fix_b")
    assert same(a, b, ("fix_scale",)) and a["fix_scale"] and not b["fix_scale"]
    assert R.judged("fix_a")[0][7] == a["sim3_in"][7] and R.judged("fix_b")[0][7] != b["sim3_in"][7] and R.pose_distance(R.judged("fix_a")[0], R.judged("fix_b")[0]) > 1000 * R.TOL
    for pair in R.PAIRS:
        assert all(k in R.CASES for k in pair)


def test_the_knobs_default_to_the_reference():
    for name in ("budget10", "budget5", "n13_3out"):
        c, (pose, removed, n_in, st) = R.case(name), R.judged(name)
        again = R.optimize_sim3(c, stage2_budget=10 if st["nbad1"] > 0 else 5, mutate=None)
        assert again[0].tobytes() == pose.tobytes() and np.array_equal(again[1], removed) and again[2] == n_in and np.array_equal(again[3]["trace"], st["trace"])
    with pytest.raises(AssertionError):
        R.optimize_sim3(R.case("n10"), mutate="no_such_variant")


def test_order_sensitivity_constants():
    """The constants of the restatement module are what reordering the correspondences gives (the way D_REF was obtained, over R.ORDERS), and every tolerance is ten times its figure."""
    d_sys0, d_chi, d_lambda = R.measure_order_sensitivity()
    for name in R.TRACED:
        f = R.order_figures(name)
        print("%-18s sys0 %.2e  prefix %2d of %2d  chi %.2e  lambda %.2e" % (name, f["sys0"], f["prefix"], len(R.judged(name)[3]["trace"]), max(f["chi"][:f["prefix"]] + [0]), max(f["lambda"][:f["prefix"]] + [0])))
    print("D_SYS0 = %r, D_CHI = %r, D_LAMBDA = %r" % (d_sys0, d_chi, d_lambda))
    assert 0.5 * R.D_SYS0 <= d_sys0 <= R.D_SYS0 and 0.5 * R.D_CHI <= d_chi <= R.D_CHI and 0.5 * R.D_LAMBDA <= d_lambda <= R.D_LAMBDA
    d_exp = float(R.exp_judged()[1].max())
    print("D_EXP = %r" % d_exp)
    assert 0.5 * R.D_EXP <= d_exp <= R.D_EXP
    assert R.SYS0_TOL == 10 * R.D_SYS0 and R.EXP_TOL == 10 * R.D_EXP and (R.exp_judged()[2] <= R.EXP_TOL).all() and (R.exp_judged()[2] >= 10 * 2.0 ** -52).all()
    assert R.TRACED == tuple(k for k in R.CASES if k != "n0")


# cases that converge quadratically have three decisive trials (gains of about 0.8, 1e-2 and 1e-6; "scale_1" two) and a next one whose gain, 1e-10, is no more than 100 x
# the 1e-11 by which chi2 moves with the summation order: they are walked as far as they go.  The cases below carry the trace comparison past the first iteration's pattern.
LONG = ("n9", "n2000", "outliers_10_more", "zero_weights", "all_outliers", "n13_3out", "behind", "budget10", "budget5", "th2_5.991", "k_a", "k_b")


def test_decisive_prefixes():
    for name in R.TRACED:
        f, t = R.order_figures(name), R.judged(name)[3]["trace"]
        assert 2 <= f["prefix"] <= f["common"] <= len(t) and (f["prefix"] >= 3 or name == "scale_1"), name
        for i in range(f["prefix"]):
            assert t[i][5] == 0.0 or f["gain"][i] >= 100 * f["chi"][i] >= 100 * R.D_SYS0, (name, i)
    for name in LONG:
        assert R.order_figures(name)["prefix"] >= 4, name
    assert set(R.NEW_CASES) - set(LONG) == {"fix_clean", "exact", "th2_7.815", "th2_20", "fix_a", "fix_b"}
    for name in ("budget10", "budget5"):  # the prefix reaches into the stage whose budget the case is about
        f, t = R.order_figures(name), R.judged(name)[3]["trace"]
        assert int((t[:f["prefix"], 0] == 1).sum()) >= 2, name
    assert R.order_figures("zero_weights")["prefix"] == 20


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_each_mutant_leaves_the_tolerance(mutant):
    """A bug the end pose forgives must not be forgiven by system0 and the decisive prefix: on some case it is 100 times outside the tolerance the device is held to."""
    caught, forgiven = [], []
    for name in R.TRACED:
        pose, _, _, st = R.optimize_sim3(R.case(name), mutate=mutant)
        w = R.compare_way(name, st["system0"], st["trace"])
        if w["sys0"] >= 100 * R.SYS0_TOL or w["chi_ratio"] >= 100 or w["lambda_ratio"] >= 100:
            caught.append(name)
            if R.pose_distance(pose, R.judged(name)[0]) <= R.TOL:
                forgiven.append(name)
    print("%s: caught on %d of %d cases; within TOL at the end, so invisible before, on %s" % (mutant, len(caught), len(R.TRACED), forgiven))
    assert len(caught) >= 5 and set(caught) & set(R.NEW_CASES) and forgiven


def test_exp_updates_reach_every_branch_and_both_sides_of_eps():
    U = R.EXP_UPDATES
    lo, hi = np.nextafter(R.EPS, 0.0), np.nextafter(R.EPS, 1.0)
    assert not U[0].any() and lo < R.EPS < hi
    br = [R.sim3_exp_branch(list(u)) for u in U]
    assert set(br) == set(R.EXP_BRANCHES)
    for s in (lo, R.EPS, hi, -lo, -R.EPS, -hi):
        assert (U[:, 6] == s).any()
    for u, b in zip(U, br):
        if abs(u[6]) in (lo, R.EPS, hi):
            assert b.startswith("sigma0") == (abs(u[6]) == lo)
    theta = np.array([np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) for u in U])
    for axis in range(3):  # single-axis rotations: theta is |omega| exactly, so the three values sit on eps and one ulp either side of it
        for v, small in ((lo, True), (R.EPS, False), (hi, False)):
            rows = [i for i in range(len(U)) if U[i][axis] == v and theta[i] == v]
            assert rows and all(br[i].endswith("theta0") == small for i in rows)
    assert ((theta > 0.5 * R.EPS) & (theta < 2 * R.EPS) & (np.count_nonzero(U[:, :3], axis=1) >= 2)).any()  # and through the sum of squares
    qb = [R.quat_branch(list(u)) for u in U[-8:]]
    assert qb[:6] == ["i0", "i0", "i1", "i1", "i2", "i2"] and set(qb[6:]) <= {"i0", "i1"} and R.quat_branch(list(U[1])) == "t>0"
    assert np.allclose(theta[-8:], np.pi - 1e-3, rtol=1e-15)
    want, d, tol = R.exp_judged()
    assert np.isfinite(want).all() and want[0].tolist() == [0, 0, 0, 0, 0, 0, 1, 1]
