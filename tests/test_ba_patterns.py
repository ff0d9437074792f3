"""CPU: every graph of tests/ba_patterns.py has the shape it is named for and is a fair parity input -- the oracle's run on it is finite, its chi2
falls, and on the metamorphic pairs (a graph and the same graph with relabelled cameras) the oracle itself takes the same LM decisions.  The ids
carry each pattern's (C, Bc): C free cameras, Bc the band half-width cs_ba_create would compute."""
import numpy as np
import pytest

from tests import ba_patterns as bp

ITERS = 10
_runs = {}


def _run(oracle, name):
    if name not in _runs:
        d = bp.build(name)
        _runs[name] = (d, oracle.ba_optimize(d, ITERS))
    return _runs[name]


@pytest.mark.parametrize("name", list(bp.CASES), ids=["%s-C%d-Bc%d" % (n, *bp.CASES[n][1]) for n in bp.CASES])
def test_pattern_shape_and_oracle_run(oracle, name):
    d, (cam, pts, cub, st) = _run(oracle, name)
    assert bp.band_shape(d) == bp.CASES[name][1]
    assert all(np.isfinite(x).all() for x in (cam, pts, cub)) and np.isfinite(st["chi2_trace"]).all() and np.isfinite(st["chi2_final"])
    assert st["iterations"] >= 1 and st["lm_trials"] >= st["iterations"]
    assert st["chi2_final"] < st["chi2_init"]
    fixed = np.asarray(d["cam_fixed"]) != 0
    assert np.allclose(cam[fixed], np.asarray(d["cam_pose"])[fixed], rtol=0, atol=1e-14), "fixed cameras do not move (the quaternion comes back renormalised)"


@pytest.mark.parametrize("name", list(bp.PAIRS))
def test_oracle_takes_the_same_lm_decisions_on_both_labellings(oracle, name):
    """Also the measurement behind the bounds of tests/test_ba_edges_gpu.py: how far the oracle moves against itself when only the camera order changes.
    Measured: chain30 cameras 2.9e-12, points 8.8e-12, chi2 trace 3.6e-14 relative; chain30_cub4 cameras 1.2e-6, points 6.5e-6, cuboids 2.7e-6, trace
    3.0e-8 relative (numeric cuboid Jacobians); outliers cameras 2.9e-10, points 1.5e-11, trace 7.7e-15 relative.  The oracle's lm_trials is the same on
    both members of every pair, the outlier graph included, so the GPU tests compare lm_trials on all of them."""
    other = bp.PAIRS[name][0]
    perm = bp.perm_of(name)
    da, (ca, pa, ua, sa) = _run(oracle, name)
    db, (cb, pb, ub, sb) = _run(oracle, other)
    assert np.array_equal(np.asarray(db["cam_pose"])[perm], da["cam_pose"]) and np.array_equal(perm[da["obs_cam"]], db["obs_cam"])
    assert oracle.ba_errors(da)[0] == pytest.approx(oracle.ba_errors(db)[0], rel=1e-13), "the same problem"
    assert sa["iterations"] == sb["iterations"] and sa["lm_trials"] == sb["lm_trials"]
    tr = np.abs(np.array(sa["chi2_trace"]) / np.array(sb["chi2_trace"]) - 1).max()
    print("%s: oracle vs oracle under permute_cameras: cameras %.2e points %.2e cuboids %.2e chi2 trace %.2e rel"
          % (name, np.abs(ca - cb[perm]).max(), np.abs(pa - pb).max(), np.abs(ua - ub).max() if len(ua) else 0.0, tr))
    loose = len(ua) > 0  # numeric-Jacobian noise of the cuboid edges (tests/test_ba_gpu.py::test_lm_trajectory)
    assert tr <= (1e-4 if loose else 1e-9)
    assert np.abs(ca - cb[perm]).max() <= (1e-4 if loose else 1e-8) and np.abs(pa - pb).max() <= (1e-4 if loose else 1e-7)


def test_transforms_do_what_they_are_named_for(oracle):
    d = bp.chain30(4)
    before = {k: np.array(v, copy=True) for k, v in d.items() if isinstance(v, np.ndarray)}
    # band_shape against the definition, block by block
    idx = bp.free_index(d)
    assert idx[0] == -1 and np.array_equal(idx[1:], np.arange(29))
    want = 0
    for cams, owner in ((d["obs_cam"], d["obs_point"]), (d["cobs_cam"], d["cobs_cuboid"])):
        for o in np.unique(owner):
            i = idx[cams[owner == o]]; i = i[i >= 0]
            if len(i):
                want = max(want, int(i.max() - i.min()))
    assert bp.band_shape(d) == (29, want)
    many = bp.fix_cameras(d, range(1, 30))
    many["cam_fixed"][5] = 0
    assert bp.band_shape(many) == (1, 0) and bp.free_index(many)[5] == 0, "255 fixed-camera flags of uint8 must not wrap"
    # permute_cameras
    p2, perm = bp.permute_cameras(d, 1)
    assert sorted(perm) == list(range(30)) and not np.array_equal(perm, np.arange(30))
    assert np.array_equal(p2["cam_pose"][perm], d["cam_pose"]) and np.array_equal(p2["cam_fixed"][perm], d["cam_fixed"]) and np.array_equal(p2["cam_true"][perm], d["cam_true"])
    assert np.array_equal(p2["obs_cam"], perm[d["obs_cam"]]) and np.array_equal(p2["cobs_cam"], perm[d["cobs_cam"]]) and p2["cam_fixed"][perm[0]] == 1
    # add_loop_edges: 25 landmarks x 3 cameras, correct geometry (the new observations reproject within the pixel noise from the true state)
    lo = bp.add_loop_edges(bp.chain30(), 25, (1, 2, 3), 2, last=5)
    base = bp.chain30()
    assert len(lo["obs_cam"]) == len(base["obs_cam"]) + 75 and np.all(np.diff(lo["obs_point"]) >= 0)
    assert bp.band_shape(lo)[1] > 20 >= bp.band_shape(base)[1]
    truth = dict(lo); truth["cam_pose"] = lo["cam_true"]; truth["points"] = lo["points_true"]
    new = np.ones(len(lo["obs_cam"]), bool)
    seen = set(zip(base["obs_cam"].tolist(), base["obs_point"].tolist()))
    for q, (c, p) in enumerate(zip(lo["obs_cam"].tolist(), lo["obs_point"].tolist())):
        new[q] = (c, p) not in seen
    assert new.sum() == 75 and set(lo["obs_cam"][new].tolist()) == {1, 2, 3}
    far = np.unique(lo["obs_point"][new])
    assert len(far) == 25 and all(base["obs_cam"][base["obs_point"] == p].min() >= 15 for p in far), "landmarks of the far end of the chain"
    eo = oracle.ba_errors(truth)[1]
    assert np.abs(eo[new, :2]).max() < 6.0 and np.abs(eo[new, :2]).std() > 0.3, "1 px noise around the true projection"
    # fix_cameras / keep_observations / cuboids_seen_only_by / with_outliers
    f = bp.fix_cameras(d, [3, 4, 9])
    assert np.flatnonzero(f["cam_fixed"]).tolist() == [0, 3, 4, 9] and bp.band_shape(f)[0] == 26
    mask = np.arange(len(d["obs_cam"])) % 2 == 0
    k = bp.keep_observations(d, mask)
    assert all(np.array_equal(k[n], d[n][mask]) for n in ("obs_cam", "obs_point", "obs_uv", "obs_inv_sigma2"))
    cams0 = np.unique(d["cobs_cam"][d["cobs_cuboid"] == 0])
    s = bp.cuboids_seen_only_by(d, cams0[:2], cuboids=[0])
    assert np.unique(s["cobs_cam"][s["cobs_cuboid"] == 0]).tolist() == cams0[:2].tolist()
    assert all((s["cobs_cuboid"] == q).sum() == (d["cobs_cuboid"] == q).sum() for q in (1, 2, 3)) and len(s["cobs_bbox"]) == len(s["cobs_cam"]) == len(s["cobs_info"])
    w = bp.with_outliers(d, 0.2, 40.0, 3)
    moved = np.abs(w["obs_uv"] - d["obs_uv"]).max(1) > 0
    assert moved.sum() == round(0.2 * len(moved)) and 30 < (w["obs_uv"] - d["obs_uv"])[moved].std() < 50
    for name, v in before.items():
        assert np.array_equal(d[name], v), "the transforms leave their input alone: " + name


def test_degenerate_patterns_are_degenerate():
    d = bp.build("starved_landmarks")
    n = np.bincount(d["obs_point"], minlength=len(d["points"]))
    assert (n == 0).sum() >= 30 and (n == 1).sum() >= 50 and (n >= 2).sum() >= 100
    d = bp.build("dead_cuboid")
    obs0 = d["cobs_cam"][d["cobs_cuboid"] == 0]
    assert len(obs0) == 2 and d["cam_fixed"][obs0].all(), "cuboid 0: every observing camera is fixed"
    assert any((d["cam_fixed"][d["cobs_cam"][d["cobs_cuboid"] == q]] == 0).any() for q in (1, 2)), "beside a live cuboid"
    d = bp.build("all_fixed_cuboids_only")
    assert d["cam_fixed"].all() and len(d["cuboid_pose"]) == 3 and len(d["cobs_cam"]) > 0
    d = bp.build("one_free")
    assert np.flatnonzero(d["cam_fixed"] == 0).tolist() == [6]
    d = bp.build("chain30_scrambled")
    assert d["cam_fixed"][0] == 0 and d["cam_fixed"].sum() == 1, "the fixed camera is no longer index 0"
    for name in ("twist_C29_Bc4", "twist_C30_Bc4", "ladder_Bc20", "long_Bc20"):
        d = bp.build(name)
        assert (np.bincount(d["obs_cam"], minlength=len(d["cam_pose"]))[d["cam_fixed"] == 0] > 0).all(), "every free camera observes"
