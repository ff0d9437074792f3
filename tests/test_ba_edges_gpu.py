"""GPU parity of the BA's reduced solve off the default chain: band half-widths 1..21 (MFMA limit, scalar trailing update, second and third back-solve
accumulators, fall-back to the sparse path), the seams between the four solver paths, scrambled and looped graphs with real fill-in, small and degenerate
systems, gross outliers -- each against the CPU oracle, each asserting through the kernel-timing counters which solver kernels ran.
The graphs are those of tests/ba_patterns.py, vetted on the CPU by tests/test_ba_patterns.py.

Bounds (tests/test_ba_gpu.py::test_lm_trajectory, ::test_two_sided_band_solver_agrees_with_one_sided): cuboid-free chi2 trace rtol 1e-9, cameras 1e-8,
points 1e-7; with cuboids 1e-4 (numeric-Jacobian noise); final chi2 within the north-star 1e-5 everywhere."""
import numpy as np
import pytest

from cube_slam_amd import _lib
from cube_slam_amd.ba import BundleAdjuster
from tests import ba_patterns as bp

pytestmark = pytest.mark.gpu
REL = 1e-5
PATHS = {"band1": {"ba_band_chol"}, "twist": {"ba_band_twist_factor", "ba_band_mid", "ba_band_twist_back"}, "cr": {"ba_cr_eliminate", "ba_cr_back"},
         "sparse": {"ba_chol_fill", "ba_chol_factor", "ba_chol_solve"}}
SOLVER_KERNELS = sorted(set().union(*PATHS.values()))
_ref = {}


def _oracle_run(oracle, name, iters, d=None):
    if (name, iters) not in _ref:
        _ref[(name, iters)] = oracle.ba_optimize(bp.build(name) if d is None else d, iters)
    return _ref[(name, iters)]


def _device_run(ctx, monkeypatch, d, iters, solver, path):
    """one BundleAdjuster run under CUBESLAM_BA_SOLVER=solver (None: the library's own choice); asserts that exactly the solver kernels of `path` ran"""
    if solver is None:
        monkeypatch.delenv("CUBESLAM_BA_SOLVER", raising=False)
    else:
        monkeypatch.setenv("CUBESLAM_BA_SOLVER", solver)
    ctx.timing(True); ctx.timing_reset()
    try:
        ba = BundleAdjuster(d, ctx=ctx)
        st = ba.optimize(iters)
        out = ba.read()
        ran = {k for k in SOLVER_KERNELS if ctx.timing_get(k)[1] > 0}
        ba.close()
    finally:
        ctx.timing(False)
    assert ran == PATHS[path], "CUBESLAM_BA_SOLVER=%s: expected the %s path, ran %s" % (solver, path, sorted(ran))
    return st, out


def _compare(tag, got, ref, cuboids, cam_map=None, tol=None):
    """device (st, (cam, pts, cub)) against oracle (cam, pts, cub, st); cam_map: device camera order -> reference order.  Prints every figure first."""
    st, (cam, pts, cub) = got
    rcam, rpts, rcub, rst = ref
    if cam_map is not None:
        cam = cam[cam_map]
    t_tr, t_cam, t_pts = tol or ((1e-4, 1e-4, 1e-4) if cuboids else (1e-9, 1e-8, 1e-7))
    n = min(len(st["chi2_trace"]), len(rst["chi2_trace"]))
    d_tr = float(np.abs(np.array(st["chi2_trace"][:n]) / np.array(rst["chi2_trace"][:n]) - 1).max()) if n else 0.0
    d_cam, d_pts = float(np.abs(cam - rcam).max()), float(np.abs(pts - rpts).max())
    d_cub = float(np.abs(cub - rcub).max()) if len(rcub) else 0.0
    d_fin = abs(st["chi2_final"] - rst["chi2_final"]) / rst["chi2_final"]
    print("BA-EDGES %-44s it %d/%d trials %d/%d  trace %.2e  cam %.2e  pts %.2e  cub %.2e  final %.2e"
          % (tag, st["iterations"], rst["iterations"], st["lm_trials"], rst["lm_trials"], d_tr, d_cam, d_pts, d_cub, d_fin))
    assert st["iterations"] == rst["iterations"] and st["lm_trials"] == rst["lm_trials"], tag
    assert np.isfinite(cam).all() and np.isfinite(pts).all()
    assert d_tr <= t_tr, (tag, d_tr)
    assert d_fin <= REL, (tag, d_fin)
    assert d_cam <= t_cam and d_pts <= t_pts and d_cub <= 1e-4, (tag, d_cam, d_pts, d_cub)


# ----------------------------------------------------------------------------------------------- a. band-width ladder
@pytest.mark.parametrize("Bc", [1, 9, 10, 11, 16, 17, 20])
def test_band_width_ladder(ctx, oracle, monkeypatch, Bc):
    """(C, Bc) = (47, Bc), cuboid-free.  Bc = 10: the MFMA trailing update at its limit (ten tiles, 60-row panel); Bc >= 11: the scalar trailing update
    in several passes; Bc >= 9 / >= 17: band_back's second / third accumulator; Bc = 20: the largest LDS request (133 KB).  Forced onto ba_band_chol and
    under the library's own choice: nested dissection at Bc = 1 (C >= 16 Bc), ba_band_chol above (C < 6 (Bc + 1))."""
    name = "ladder_Bc%d" % Bc
    d = bp.build(name)
    assert bp.band_shape(d) == (47, Bc)
    ref = _oracle_run(oracle, name, 6, d)
    _compare(name + " =band1", _device_run(ctx, monkeypatch, d, 6, "band1", "band1"), ref, False)
    _compare(name + " default", _device_run(ctx, monkeypatch, d, 6, None, "cr" if Bc == 1 else "band1"), ref, False)


def test_two_sided_chain_at_the_widest_band(ctx, oracle, monkeypatch):
    """(C, Bc) = (126, 20): C >= 6 (Bc + 1), so =band and the default take the two-sided chain; ba_band_mid factors its sized limit N = 6 Bc = 120"""
    d = bp.build("long_Bc20")
    assert bp.band_shape(d) == (126, 20)
    ref = _oracle_run(oracle, "long_Bc20", 5, d)
    _compare("long_Bc20 =band", _device_run(ctx, monkeypatch, d, 5, "band", "twist"), ref, False)
    _compare("long_Bc20 default", _device_run(ctx, monkeypatch, d, 5, None, "twist"), ref, False)
    _compare("long_Bc20 =band1", _device_run(ctx, monkeypatch, d, 5, "band1", "band1"), ref, False)


# ----------------------------------------------------------------------------------------------- b. fall-back at Bc = 21
def test_band_wider_than_the_lds_window_falls_back_to_sparse(ctx, oracle, monkeypatch):
    """(C, Bc) = (47, 21) > BAND_MAX = 20: the default runs the sparse block Cholesky and no band kernel; =band and =band1 are refused with CS_ERR_CAPACITY"""
    d = bp.build("ladder_Bc21")
    assert bp.band_shape(d) == (47, 21)
    _compare("ladder_Bc21 default", _device_run(ctx, monkeypatch, d, 6, None, "sparse"), _oracle_run(oracle, "ladder_Bc21", 6, d), False)
    for solver in ("band", "band1"):
        monkeypatch.setenv("CUBESLAM_BA_SOLVER", solver)
        with pytest.raises(_lib.CubeSlamError, match="CS_ERR_CAPACITY"):
            BundleAdjuster(d, ctx=ctx)
    d20 = bp.build("ladder_Bc20")  # one narrower: still a band, and =sparse on it agrees too
    _compare("ladder_Bc20 =sparse", _device_run(ctx, monkeypatch, d20, 6, "sparse", "sparse"), _oracle_run(oracle, "ladder_Bc20", 6, d20), False)


# ----------------------------------------------------------------------------------------------- c. nested dissection
@pytest.mark.parametrize("Bc", [1, 3, 9, 10])
def test_nested_dissection_at_odd_half_widths(ctx, oracle, monkeypatch, Bc):
    """=cr at (C, Bc) = (47, Bc): super-blocks of 2, 4, 10, 10 cameras, odd Bc padded with explicit zeros inside the super-block, C no multiple of it"""
    name = "ladder_Bc%d" % Bc
    d = bp.build(name)
    assert bp.band_shape(d) == (47, Bc) and 47 % (2, 4, 6, 8, 10)[(Bc - 1) // 2] != 0
    _compare(name + " =cr", _device_run(ctx, monkeypatch, d, 6, "cr", "cr"), _oracle_run(oracle, name, 6, d), False)


def test_nested_dissection_at_its_shortest_chain(ctx, oracle, monkeypatch):
    """Bc = 9: C = 36 = 4 Bc is the least nested dissection takes; at C = 35 =cr quietly runs a band kernel and is still right"""
    d = bp.build("cr_C36_Bc9")
    assert bp.band_shape(d) == (36, 9)
    _compare("cr_C36_Bc9 =cr", _device_run(ctx, monkeypatch, d, 6, "cr", "cr"), _oracle_run(oracle, "cr_C36_Bc9", 6, d), False)
    d = bp.build("cr_C35_Bc9")
    assert bp.band_shape(d) == (35, 9)
    _compare("cr_C35_Bc9 =cr", _device_run(ctx, monkeypatch, d, 6, "cr", "band1"), _oracle_run(oracle, "cr_C35_Bc9", 6, d), False)


# ----------------------------------------------------------------------------------------------- d. twist seam
@pytest.mark.parametrize("C", [29, 30])
def test_either_side_of_the_two_sided_threshold(ctx, oracle, monkeypatch, C):
    """Bc = 4: the chain is eliminated from both ends from C = 6 (Bc + 1) = 30 on, by the default and by =band alike (C < 16 Bc: no nested dissection)"""
    name = "twist_C%d_Bc4" % C
    d = bp.build(name)
    assert bp.band_shape(d) == (C, 4)
    ref = _oracle_run(oracle, name, 6, d)
    for solver in (None, "band"):
        _compare("%s %s" % (name, solver or "default"), _device_run(ctx, monkeypatch, d, 6, solver, "twist" if C >= 30 else "band1"), ref, False)


# ----------------------------------------------------------------------------------------------- e. scrambled and looped graphs
@pytest.mark.parametrize("name", ["chain30", "chain30_cub4"])
def test_scrambled_camera_order_is_the_same_problem(ctx, oracle, monkeypatch, name):
    """permute_cameras turns the 30-key-frame chain (band path) into a graph of half-width 26: the sparse path with genuine minimum-degree fill, the fixed
    camera no longer at index 0.  Both runs against the oracle, and the sparse result, un-permuted, against the band result.
    Device against device the bound is 100 x what the oracle moves against itself under the same relabelling (tests/test_ba_patterns.py: cameras 2.9e-12,
    points 8.8e-12, chi2 trace 3.6e-14 relative without cuboids), i.e. cameras 2.9e-10, points 8.8e-10, trace 3.6e-12; with 4 cuboids the oracle moves by
    1.2e-6 / 6.5e-6 / 3.0e-8, 100 x that is beyond the project's cuboid tolerance 1e-4, which therefore holds."""
    cuboids = name.endswith("cub4")
    plain, other = bp.build(name), bp.build(bp.PAIRS[name][0])
    perm = bp.perm_of(name)
    assert bp.band_shape(plain)[1] <= 9 and bp.band_shape(other) == (29, 26)
    a = _device_run(ctx, monkeypatch, plain, 8, None, "band1")
    b = _device_run(ctx, monkeypatch, other, 8, None, "sparse")
    _compare(name + " plain, band", a, _oracle_run(oracle, name, 8, plain), cuboids)
    _compare(name + " scrambled, sparse", b, _oracle_run(oracle, bp.PAIRS[name][0], 8, other), cuboids)
    _compare(name + " sparse(scrambled) vs band(plain)", b, (*a[1], a[0]), cuboids, cam_map=perm, tol=None if cuboids else (3.6e-12, 2.9e-10, 8.8e-10))
    if not cuboids:  # the Schur slots of far-apart pairs, apart from the factorisation
        ba = BundleAdjuster(other, ctx=ctx)
        H, b_ = ba.reduced_dense(2.5)
        ba.close()
        rH, rb = oracle.ba_reduced_dense(other, 0, len(other["points"]), True, 2.5)
        assert np.allclose(H, rH, rtol=1e-9, atol=1e-10 * np.abs(rH).max()) and np.allclose(b_, rb, rtol=1e-9, atol=1e-10 * np.abs(rb).max())


def test_loop_edges_take_the_sparse_path(ctx, oracle, monkeypatch):
    """25 landmarks of the far end of the 30-key-frame chain also seen by cameras 1-3 (half-width 22): a loop closure.  reduced_dense separates a fault in
    the Schur slots of the far-apart camera pairs from one in the factorisation."""
    d = bp.build("chain30_loop")
    assert bp.band_shape(d) == (29, 22)
    monkeypatch.delenv("CUBESLAM_BA_SOLVER", raising=False)
    ba = BundleAdjuster(d, ctx=ctx)
    H, b = ba.reduced_dense(2.5)
    ba.close()
    rH, rb = oracle.ba_reduced_dense(d, 0, len(d["points"]), True, 2.5)
    far = [(i, j) for i in range(3) for j in range(15, 29) if np.abs(rH[6 * i:6 * i + 6, 6 * j:6 * j + 6]).max() > 0]
    assert len(far) >= 6, "the loop edges couple cameras 1-3 with the far end"
    print("BA-EDGES chain30_loop reduced_dense: H %.2e of %.2e, b %.2e of %.2e" % (np.abs(H - rH).max(), np.abs(rH).max(), np.abs(b - rb).max(), np.abs(rb).max()))
    assert np.allclose(H, rH, rtol=1e-9, atol=1e-10 * np.abs(rH).max()) and np.allclose(b, rb, rtol=1e-9, atol=1e-10 * np.abs(rb).max())
    _compare("chain30_loop default", _device_run(ctx, monkeypatch, d, 8, None, "sparse"), _oracle_run(oracle, "chain30_loop", 8, d), False)
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_CAPACITY"):
        monkeypatch.setenv("CUBESLAM_BA_SOLVER", "band")
        BundleAdjuster(d, ctx=ctx)


# ----------------------------------------------------------------------------------------------- f. small and degenerate
@pytest.mark.parametrize("n_kf", [2, 3, 4, 7])
def test_systems_smaller_than_the_band_window(ctx, oracle, monkeypatch, n_kf):
    """C = 1, 2, 3, 6 free cameras that all share landmarks (Bc = C - 1): fewer columns than the LDS ring has slots.  One free camera has half-width 0,
    which the library widens to 1 (band_back's chunks would hold no column)."""
    name = "tiny_kf%d" % n_kf
    d = bp.build(name)
    assert bp.band_shape(d) == (n_kf - 1, n_kf - 2)
    ref = _oracle_run(oracle, name, 6, d)
    _compare(name + " default", _device_run(ctx, monkeypatch, d, 6, None, "band1"), ref, False)
    _compare(name + " =sparse", _device_run(ctx, monkeypatch, d, 6, "sparse", "sparse"), ref, False)


def test_fixed_cameras_in_the_middle_and_one_free_camera(ctx, oracle, monkeypatch):
    """14 key frames, 3 cuboids (1e-4: numeric cuboid Jacobians).  Cameras 0, 3, 4, 9 fixed: (C, Bc) = (10, 6), the free-camera index skips the fixed ones
    and their camera-cuboid blocks are dead; camera 6 alone free: (1, 0)"""
    for name, shape in (("fixed_mid", (10, 6)), ("one_free", (1, 0))):
        d = bp.build(name)
        assert bp.band_shape(d) == shape
        ref = _oracle_run(oracle, name, 6, d)
        _compare(name + " default", _device_run(ctx, monkeypatch, d, 6, None, "band1"), ref, True)
        _compare(name + " =sparse", _device_run(ctx, monkeypatch, d, 6, "sparse", "sparse"), ref, True)
        fixed = d["cam_fixed"] != 0
        monkeypatch.delenv("CUBESLAM_BA_SOLVER", raising=False)
        ba = BundleAdjuster(d, ctx=ctx)
        ba.optimize(2)
        assert np.allclose(ba.read()[0][fixed], d["cam_pose"][fixed], rtol=0, atol=1e-14), "fixed cameras stay"
        ba.close()


def test_all_cameras_fixed_cuboids_only(ctx, oracle, monkeypatch):
    """C = 0: the pose blocks are the three cuboids alone; no band to speak of, the sparse path runs over the cuboid blocks; =band is refused"""
    d = bp.build("all_fixed_cuboids_only")
    assert bp.band_shape(d) == (0, 0)
    _compare("all_fixed default", _device_run(ctx, monkeypatch, d, 6, None, "sparse"), _oracle_run(oracle, "all_fixed_cuboids_only", 6, d), True)
    monkeypatch.setenv("CUBESLAM_BA_SOLVER", "band")
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_CAPACITY"):
        BundleAdjuster(d, ctx=ctx)


def test_cuboid_whose_observing_cameras_are_all_fixed(ctx, oracle, monkeypatch):
    """cuboid 0 is seen by two cameras only and both are fixed (dead Schur blocks; it still moves through its point-cuboid edges), cuboid 1 by no camera
    at all, cuboid 2 by live cameras: (C, Bc) = (11, 9)"""
    d = bp.build("dead_cuboid")
    assert bp.band_shape(d) == (11, 9)
    ref = _oracle_run(oracle, "dead_cuboid", 6, d)
    _compare("dead_cuboid default", _device_run(ctx, monkeypatch, d, 6, None, "band1"), ref, True)
    _compare("dead_cuboid =sparse", _device_run(ctx, monkeypatch, d, 6, "sparse", "sparse"), ref, True)


def test_landmarks_with_one_observation_and_with_none(ctx, oracle, monkeypatch):
    """every third landmark keeps one observation (a rank-2 point block that only the damping makes invertible), every seventh none: (C, Bc) = (13, 9)"""
    d = bp.build("starved_landmarks")
    assert bp.band_shape(d) == (13, 9)
    ref = _oracle_run(oracle, "starved_landmarks", 6, d)
    _compare("starved default", _device_run(ctx, monkeypatch, d, 6, None, "band1"), ref, False)
    _compare("starved =sparse", _device_run(ctx, monkeypatch, d, 6, "sparse", "sparse"), ref, False)
    unseen = np.bincount(d["obs_point"], minlength=len(d["points"])) == 0
    monkeypatch.delenv("CUBESLAM_BA_SOLVER", raising=False)
    ba = BundleAdjuster(d, ctx=ctx)
    ba.optimize(3)
    assert unseen.sum() >= 30 and np.array_equal(ba.read()[1][unseen], d["points"][unseen]), "a landmark nobody observes stays where it is"
    ba.close()


# ----------------------------------------------------------------------------------------------- g. robust kernel under load
def test_gross_outliers(ctx, oracle, monkeypatch):
    """20 % of the observations moved by 40 px on the 14-key-frame graph, 10 iterations, plain and scrambled.  The oracle's own lm_trials is the same on
    both labellings (tests/test_ba_patterns.py), so lm_trials is compared here, not only chi2 and the estimates."""
    for name, path in (("outliers", "band1"), ("outliers_scrambled", "band1")):
        d = bp.build(name)
        ba = BundleAdjuster(d, ctx=ctx)
        chi, eo, _, _ = ba.errors()
        ba.close()
        rchi, reo, _, _ = oracle.ba_errors(d)
        e2 = (reo ** 2).sum(1) * d["obs_inv_sigma2"]
        assert (e2 > d["huber_mono"] ** 2).mean() > 0.15, "the robust branch carries a real share of the edges"
        assert np.allclose(eo, reo, rtol=1e-12, atol=1e-11) and abs(chi - rchi) <= 1e-11 * rchi
        ref = _oracle_run(oracle, name, 10, d)
        _compare(name + " default", _device_run(ctx, monkeypatch, d, 10, None, path), ref, False)
        _compare(name + " =sparse", _device_run(ctx, monkeypatch, d, 10, "sparse", "sparse"), ref, False)
