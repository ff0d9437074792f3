"""CPU proof that no window of tests/badyn_patterns.py is vacuous: the sized windows have the pose-system size they claim, the list lengths the device
code forks on are all reached (restated from the rule in badyn_patterns.list_lengths), the rejected-trial windows make the oracle reject and keep their
accept / reject decisions under a relabelling of the object vertices, and on every window that tests/test_zx_badyn_edges_gpu.py holds to 1e-5 the oracle
moves against itself by less than 1e-6 under such a relabelling, which leaves that bar ten times over the reference's own order noise."""
import numpy as np
import pytest

from tests import badyn_patterns as bp

ITERS = 3  # of the new device cases (at six the oracle's own order noise reaches 3.5e-6 on the suite's seed 41)


@pytest.mark.parametrize("NP", sorted(bp.LADDER))
def test_sized_window_has_its_pose_system(oracle, NP):
    d = bp.build("np%d" % NP)
    fixed = d["cam_fixed"] != 0
    assert bp.pose_offsets(d)[3] == NP == 6 * (int((~fixed).sum()) + len(d["obj_pose"])) + 2 * len(d["vel"])
    assert oracle.badyn_reduced_dense(d, 1e-3)[0].shape == (NP, NP)
    free = np.nonzero(~fixed)[0]
    assert len(free) and fixed[free[0]:].any(), "a fixed camera sits behind a free one"
    assert np.isin(np.nonzero(~fixed)[0], np.concatenate([d["obs_cam"], d["dobs_cam"]])).all(), "every free camera is observed"
    _, st = bp.oracle_optimize(oracle, "np%d" % NP, ITERS)
    assert st["iterations"] == ITERS and st["chi2_final"] < 0.5 * st["chi2_init"]
    nblk, npan = bp.chol_launches(NP)
    assert (nblk, npan) == {32: (1, 0), 34: (2, 1), 64: (2, 1), 160: (5, 4), 162: (6, 5), 1042: (33, 32), 1090: (35, 34)}[NP]


def test_ladder_reaches_the_cholesky_seams():
    """rows behind the first pivot block: 128 (one panel workgroup of 128 rows, update grid 4 x 4) and 130 (two, 5 x 5); one window in (1024, 1056],
    one >= 1090; ragged last blocks of two rows"""
    assert 160 - 32 == 128 and (162 - 32 + 127) // 128 == 2 and (162 - 32 + 31) // 32 == 5
    big = sorted(n for n in bp.LADDER if n > 1024)
    assert len(big) == 2 and 1024 < big[0] <= 1056 and big[1] >= 1090
    assert 34 % 32 == 2 and 162 % 32 == 2 and 1090 % 32 == 2


def test_lists_reach_every_seam():
    ll = {name: bp.list_lengths(bp.build(name)) for name in bp.LIST_SEAMS + bp.REORDERED}
    blocks = [v for x in ll.values() for v in x["pb"].values()]
    counts = {v[0] for v in blocks}
    assert {1, 7, 8, 9, 16, 17} <= counts, sorted(counts)             # eight loads in flight: under, at, over one round; two rounds and one more
    assert {(6, 6), (6, 2), (2, 2)} == {v[1] for v in blocks}
    assert any(v[3] and not v[2] for v in blocks), "a block fed by transposed sources only"
    assert any(v[3] and v[2] for v in blocks), "a block fed by both kinds of source"
    assert {10, 11, 20, 21} <= {x["n_pg"] for x in ll.values()}       # ten gradients per workgroup
    pairs = {n for x in ll.values() for n in x["schur"].values()}
    assert min(pairs) <= 6 and {7, 8} <= pairs and max(pairs) >= 15   # seven lane groups per Schur block
    slots = {n for x in ll.values() for n in x["slots"].values()}
    assert min(slots) <= 9 and {10, 11} <= slots and max(slots) >= 21  # ten lane groups per vertex
    assert {64, 65} <= {x["L"] for x in ll.values()}                  # 64 landmarks per workgroup
    n_edges = {x["n_edges"] for x in ll.values()}
    assert min(n_edges) <= 64 and {256, 257} <= n_edges               # 64 edges per linearize workgroup, 256 per partial sum
    # the thinned vertices carry exactly what dobs_per_vertex promises
    a = ll["lists_L64_pg21"]
    for n in bp.VERTEX_COUNTS:
        assert n + 1 in {v[0] for v in a["pb"].values()} and n in a["schur"].values() and n in a["slots"].values(), n


def _block_asymmetry(oracle, d):
    """of every 6 x 6 pose block with a transposed source: max |B - B^T| in the oracle's pose system (points fixed: no Schur terms on top) over the
    largest entry of the reduced system, i.e. how far reading that block the wrong way round moves what the device test holds to 1e-8"""
    df = dict(d); df["fix_points"] = 1
    H, _ = oracle.badyn_reduced_dense(df, 0.0)
    top = np.abs(oracle.badyn_reduced_dense(d, 2e-3)[0]).max()
    return [float(np.abs(H[lo:lo + 6, hi:hi + 6] - H[lo:lo + 6, hi:hi + 6].T).max() / top) for (lo, hi), v in bp.list_lengths(df)["pb"].items() if v[3] and v[1] == (6, 6)]


def test_relabelling_puts_motion_edges_against_the_offset_order(oracle):
    for name in bp.REORDERED + ("lists_L65_pg20_mixed",):
        d = bp.build(name)
        assert (d["mot_from"] > d["mot_to"]).sum() >= 3 and (d["mot_from"] < d["mot_to"]).sum() >= 3, name
    plain = bp.build("np160")
    assert (plain["mot_from"] < plain["mot_to"]).all() and not any(v[3] for v in bp.list_lengths(plain)["pb"].values())
    # With whether_fixrotation (every window the reference builds) a motion edge's block between its two vertices is symmetric: reading it transposed or
    # not gives the same numbers.  Only the yaw-free windows can tell a dropped transposition: with object_velocity_BA_weight = 5 it moves the reduced
    # system by more than ten times the device test's bar.
    sym = _block_asymmetry(oracle, bp.build("reordered_np136"))
    assert len(sym) >= 3 and max(sym) == 0.0
    for name in ("reordered_np160_yaw", "lists_L65_pg20_mixed"):
        asym = _block_asymmetry(oracle, bp.build(name))
        assert len(asym) >= 3 and min(asym) > 1e-7, (name, asym)


@pytest.mark.parametrize("name", sorted(bp.REJECTED))
def test_rejected_trial_window_is_stable_on_the_reference_side(oracle, name):
    iters = bp.REJECTED[name][2]
    _, st = bp.oracle_optimize(oracle, name, iters)
    assert st["iterations"] == iters and st["lm_trials"] > st["iterations"]
    per_iteration = np.diff([0] + [oracle.badyn_optimize(bp.build(name), k)[1]["lm_trials"] for k in range(1, iters + 1)])
    assert per_iteration.max() >= 3, "two or more rejections in a row"
    same, d_tr, d_est, d_lam = bp.order_noise(oracle, name, iters, (1, 2, 3, 4, 5))
    print("BADYN-PATTERNS %-28s it %d trials %d per iteration %s  order noise: trace %.2e est %.2e lambda %.2e"
          % (name, st["iterations"], st["lm_trials"], [int(x) for x in per_iteration], d_tr, d_est, d_lam))
    assert same, "the accept / reject decisions survive a reordering of the sums"
    assert d_tr <= 1e-6 and d_est <= 1e-6
    # lambda_final is held to 1e-4 on the device.  Where a trial's gain ratio falls between the clamps of the update factor, lambda takes the ratio's
    # noise, amplified by chi2 over its decrease (shaken_centres(64) moves by 4e-4 under a relabelling and was dropped for it): a tenth of the bar here too
    assert d_lam <= 1e-5


@pytest.mark.parametrize("name", ["np%d" % n for n in sorted(bp.LADDER)] + list(bp.LIST_SEAMS) + list(bp.REORDERED))
def test_order_noise_is_a_tenth_of_the_device_bar(oracle, name):
    same, d_tr, d_est, d_lam = bp.order_noise(oracle, name, ITERS)
    print("BADYN-PATTERNS %-28s order noise at %d iterations: trace %.2e est %.2e lambda %.2e" % (name, ITERS, d_tr, d_est, d_lam))
    assert same and d_tr <= 1e-6 and d_est <= 1e-6 and d_lam <= 1e-5


def test_point_without_active_edge_comes_back_unchanged(oracle):
    d = bp.build("edges257_pg11_dead_point")
    p = d["dead_point"]
    rows = d["obs_point"] == p
    assert rows.sum() >= 2 and (d["obs_level"][rows] == 1).all() and (d["obs_level"][~rows] == 0).all()
    res, st = bp.oracle_optimize(oracle, "edges257_pg11_dead_point", ITERS)
    assert res["points"][p].tobytes() == d["points"][p].tobytes()
    others = np.arange(len(d["points"])) != p
    seen = np.bincount(d["obs_point"], minlength=len(d["points"])) > 0
    assert (res["points"][others & seen] != d["points"][others & seen]).any(axis=1).all(), "every other observed point moves"


def test_transforms_leave_the_problem_itself_alone(oracle):
    """relabelling is the same problem (chi2 and residuals to the last bits), a reverse twin adds its own residual, thinning drops rows only"""
    d = bp.build("np64")
    d2 = bp.reordered(d, 4)
    chi, e = oracle.badyn_errors(d)
    chi2, e2 = oracle.badyn_errors(d2)
    assert not np.array_equal(d2["obj_perm"], np.arange(len(d["obj_pose"]))) and np.isclose(chi, chi2, rtol=1e-14)
    for k in e:
        assert np.array_equal(e[k], e2[k]), k
    t = bp.thinned(d, drop_obs=[0, 5], drop_dobs=[1])
    assert len(t["obs_cam"]) == len(d["obs_cam"]) - 2 and len(t["dobs_uv"]) == len(d["dobs_uv"]) - 1 and np.array_equal(t["obs_uv"][0], d["obs_uv"][1])
    r = bp.with_reverse_motion(d)
    assert len(r["mot_from"]) > len(d["mot_from"]) and len(oracle.badyn_errors(r)[1]["mot"]) == len(r["mot_from"])
