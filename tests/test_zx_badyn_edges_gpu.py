"""(Sorts beside tests/test_zx_badyn_gpu.py on purpose: the one engine with run-dependent history runs late.)
GPU parity of the dynamic-object bundle adjustment (cs_ba_dyn_*, cube_slam_amd/csrc/badyn.hip) at the seams of its device code, each case against the
oracle on the same window and each asserting through the kernel-timing counters which kernels ran and how often:
the blocked Cholesky at pose systems of 32, 34, 64, 160, 162, 1042 and 1090 scalars; object vertices relabelled against time (transposed sources of
badyn_gather_blocks); gather, Schur and slot lists of exact lengths and a static point without an active edge; windows on which Levenberg-Marquardt
rejects trials (pop, growth of lambda, repeated solves on one build); the stop flags; the refusal above DYN_MAX_NP.
The windows are those of tests/badyn_patterns.py, vetted on the CPU by tests/test_badyn_patterns.py.

Bars (tests/test_zx_badyn_gpu.py): chi2_init 1e-10, residuals 1e-9, reduced system 1e-8 of its largest entry, chi2 trace and every estimate 1e-5,
lambda_final 1e-4, iterations and lm_trials equal.  Every case prints what it measured before it asserts."""
import ctypes as C

import numpy as np
import pytest

from cube_slam_amd import _lib, synth
from cube_slam_amd.ba import BAStats
from cube_slam_amd.ba_dynamic import DynamicBundleAdjuster, problem_struct
from tests import badyn_patterns as bp

pytestmark = pytest.mark.gpu
ITERS = 3
COUNTED = ("badyn_errors", "badyn_linearize", "badyn_linearize_dyn", "badyn_linearize_num", "badyn_gather_blocks", "badyn_gather_grad", "badyn_gather_lm",
           "badyn_schur_init", "badyn_dinv", "badyn_bd", "badyn_schur_blocks", "badyn_schur_rhs", "badyn_chol_diag", "badyn_chol_panel", "badyn_chol_update",
           "badyn_chol_tri", "badyn_backsub", "badyn_update", "badyn_diag")


def _counts(ctx):
    return {k: ctx.timing_get(k)[1] for k in COUNTED}


def _stats(st):
    return {"iterations": st.iterations, "lm_trials": st.lm_trials, "chi2_init": st.chi2_init, "chi2_final": st.chi2_final, "lambda_final": st.lambda_final,
            "chi2_trace": list(st.chi2_trace)[:st.iterations]}


def _run(ctx, oracle, name, iters, lam=None):
    """One window on the device against the oracle: residuals, the reduced system at `lam` (None: not asked for), optimize(iters), read(), errors().
    Prints every deviation, asserts every bar and the launch counts that follow from (iterations, lm_trials, NP).  -> (stats, estimates, counts)"""
    d = bp.build(name)
    NP = bp.pose_offsets(d)[3]
    res_o, st_o = bp.oracle_optimize(oracle, name, iters)
    chi_o, e_o = oracle.badyn_errors(d)
    ctx.timing(True); ctx.timing_reset()
    try:
        ba = DynamicBundleAdjuster(d, ctx=ctx)
        chi, e = ba.errors()
        d_H = d_b = 0.0
        if lam is not None:
            H, b = ba.reduced_dense(lam)
            H_o, b_o = oracle.badyn_reduced_dense(d, lam)
            assert H.shape == H_o.shape == (NP, NP)
            d_H, d_b = bp.deviation(H, H_o), bp.deviation(b, b_o)
        st = ba.optimize(iters)
        res = ba.read()
        chi_end, _ = ba.errors()
        n = _counts(ctx)
        ba.close()
    finally:
        ctx.timing(False)
    d_res = max(float(np.abs(e[k] - e_o[k]).max()) / max(1.0, float(np.abs(e_o[k]).max())) if e_o[k].size else 0.0 for k in e_o)
    d_tr = bp.deviation(st["chi2_trace"], st_o["chi2_trace"]) if st["iterations"] == st_o["iterations"] else float("inf")
    d_est = {k: bp.deviation(res[k], res_o[k]) for k in bp.EST}
    d_lam = abs(st["lambda_final"] / st_o["lambda_final"] - 1)
    d_end = abs(chi_end / st["chi2_final"] - 1)
    print("BADYN-EDGES %-26s NP %4d it %d/%d trials %d/%d  chi2_init %.2e  residuals %.2e  H %.2e  b %.2e  trace %.2e  %s  lambda %.2e  errors() after %.2e"
          % (name, NP, st["iterations"], st_o["iterations"], st["lm_trials"], st_o["lm_trials"], abs(chi / chi_o - 1), d_res, d_H, d_b, d_tr,
             "  ".join("%s %.2e" % (k, v) for k, v in d_est.items()), d_lam, d_end))
    assert abs(chi / chi_o - 1) <= 1e-10 and abs(st["chi2_init"] / st_o["chi2_init"] - 1) <= 1e-10
    for k in e_o:
        assert e[k].shape == e_o[k].shape and np.allclose(e[k], e_o[k], rtol=1e-9, atol=1e-9), k
    assert d_H <= 1e-8 and d_b <= 1e-8
    assert st["iterations"] == st_o["iterations"] and st["lm_trials"] == st_o["lm_trials"]
    assert d_tr <= 1e-5 and max(d_est.values()) <= 1e-5, (d_tr, d_est)
    assert d_lam <= 1e-4
    assert d_end <= 1e-9, "the residuals on the device are those of the accepted state"
    # launches: one build per iteration (and one for reduced_dense, which reduces but does not factor), one solve and one update per trial
    builds, solves = st["iterations"] + (lam is not None), st["lm_trials"]
    nblk, npan = bp.chol_launches(NP)
    assert n["badyn_gather_blocks"] == builds and n["badyn_gather_grad"] == builds and n["badyn_gather_lm"] == builds
    assert n["badyn_linearize"] == builds * (len(d["obs_cam"]) > 0) and n["badyn_linearize_dyn"] == builds * (len(d["dobs_cam"]) > 0) and n["badyn_linearize_num"] == builds
    assert n["badyn_schur_init"] == solves + (lam is not None) == n["badyn_dinv"] == n["badyn_bd"] == n["badyn_schur_blocks"] == n["badyn_schur_rhs"]
    assert n["badyn_chol_diag"] == solves * nblk and n["badyn_chol_panel"] == solves * npan == n["badyn_chol_update"], (n, nblk, npan)
    assert n["badyn_chol_tri"] == solves == n["badyn_backsub"] == n["badyn_update"] and n["badyn_diag"] == 1
    return st, res, n


# ----------------------------------------------------------------------------------------------- a. solver ladder
@pytest.mark.parametrize("NP", sorted(bp.LADDER))
def test_solver_ladder(ctx, oracle, NP):
    """NP = 32: one full block, no panel or update launch; 34: a ragged last block of two rows padded with the identity; 64: two full blocks, nothing
    behind the second; 160 / 162: 128 / 130 rows behind the first block (one / two panel workgroups, update grid 4 x 4 / 5 x 5); 1042: the load and
    store loops of badyn_chol_tri take a second pass; 1090: its forward row loop and backward column loop too."""
    st, _, n = _run(ctx, oracle, "np%d" % NP, ITERS, lam=2e-3)
    assert st["iterations"] == ITERS
    assert (n["badyn_chol_panel"] == 0) == (NP == 32) and n["badyn_chol_diag"] == st["lm_trials"] * ((NP + 31) // 32)
    if NP in (34, 64):
        assert n["badyn_chol_panel"] == st["lm_trials"]


# ----------------------------------------------------------------------------------------------- b. relabelled object vertices
@pytest.mark.parametrize("name", bp.REORDERED)
def test_reordered_object_vertices(ctx, oracle, name):
    """object vertices in map order: motion edges whose `from` vertex lies behind their `to` vertex in the pose system feed badyn_gather_blocks
    transposed sources.  reordered_np136 is the suite's seed-41 window as the reference would hand it over (rotation fixed: those blocks are symmetric);
    on reordered_np160_yaw the yaw is free and a block read the wrong way round moves the reduced system by 1e-6 of its largest entry
    (tests/test_badyn_patterns.py)."""
    d = bp.build(name)
    assert (d["mot_from"] > d["mot_to"]).any()
    _run(ctx, oracle, name, ITERS, lam=2e-3)


# ----------------------------------------------------------------------------------------------- c. list seams
@pytest.mark.parametrize("name", bp.LIST_SEAMS)
def test_list_seams(ctx, oracle, name):
    """block source lists of 1, 7, 8, 9, 16, 17 entries (eight loads in flight, clamped tail), plain, transposed and mixed; 10 / 11 / 20 / 21 gradient
    targets; Schur pair lists and slot lists around 7 and 10 lane groups; 64 / 65 landmarks; <= 64, 256 and 257 edges (tests/test_badyn_patterns.py
    asserts that the set reaches each).  The static point whose observations all sit at level 1 comes back bit-unchanged."""
    d = bp.build(name)
    _, res, _ = _run(ctx, oracle, name, ITERS, lam=2e-3)
    if "dead_point" in d:
        p = d["dead_point"]
        assert res["points"][p].tobytes() == np.ascontiguousarray(d["points"][p], np.float64).tobytes(), "a point without an active edge does not move"
        assert (res["points"][np.arange(len(res["points"])) != p] != np.delete(d["points"], p, axis=0)).any()


# ----------------------------------------------------------------------------------------------- d. rejected trials
@pytest.mark.parametrize("name", sorted(bp.REJECTED))
def test_rejected_trials(ctx, oracle, name):
    """pop() of the estimates, growth of lambda, repeated solves on an unchanged build with the right-hand side and the step reused on the host, the
    retry loop -- up to three rejections in a row.  errors() after optimize() is the chi2 of the accepted state only if a pop restored everything."""
    iters = bp.REJECTED[name][2]
    st, res, n = _run(ctx, oracle, name, iters)
    assert st["lm_trials"] > st["iterations"] == iters
    assert n["badyn_errors"] >= st["lm_trials"] + 2 + 1  # every trial, the two errors() calls, and one more after each iteration that ended in a rejection
    ba = DynamicBundleAdjuster(bp.build(name), ctx=ctx)  # no floating-point atomics, pops included: the same bits again
    st2 = ba.optimize(iters)
    res2 = ba.read()
    ba.close()
    assert st2 == st
    for k in res:
        assert res2[k].tobytes() == res[k].tobytes(), k


# ----------------------------------------------------------------------------------------------- e. stop flags
def _optimize(ctx, ba, iters, flag=None):
    st = BAStats()
    _lib.check(ctx.ptr, _lib.lib().cs_ba_dyn_optimize(ctx.ptr, ba._b, iters, None if flag is None else C.byref(flag), C.byref(st)), "cs_ba_dyn_optimize")
    return _stats(st)


@pytest.mark.parametrize("kind", ["int", "bool"])
def test_stop_flag_set_before_the_call(ctx, kind):
    d = bp.build("np64")
    fresh = DynamicBundleAdjuster(d, ctx=ctx)
    start = fresh.read()  # the input estimates as cs_ba_dyn_create stores them: rotations normalised
    st_f = _optimize(ctx, fresh, 5)
    res_f = fresh.read()
    fresh.close()
    for k in ("vel", "points", "dpoints"):
        assert start[k].tobytes() == np.ascontiguousarray(d[k], np.float64).tobytes(), k
    for k in ("cam_pose", "obj_pose"):
        q = np.where(d[k][:, 6:] < 0, -d[k][:, 3:], d[k][:, 3:])  # w >= 0, unit norm (se3quat.h:331-336)
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        assert np.array_equal(start[k][:, :3], d[k][:, :3]) and np.abs(start[k][:, 3:] - q).max() <= 4e-16, k
    ba = DynamicBundleAdjuster(d, ctx=ctx)
    flag = C.c_int(1) if kind == "int" else C.c_ubyte(1)
    if kind == "bool":
        _lib.check(ctx.ptr, _lib.lib().cs_ba_dyn_set_stop_flag_bool(ba._b, C.byref(flag)), "cs_ba_dyn_set_stop_flag_bool")
    ctx.timing(True); ctx.timing_reset()
    try:
        st = _optimize(ctx, ba, 5, flag if kind == "int" else None)
        n = _counts(ctx)
    finally:
        ctx.timing(False)
    assert st["iterations"] == 0 and st["lm_trials"] == 0 and st["chi2_trace"] == []
    assert n["badyn_linearize"] == 0 and sum(n.values()) == 0, n
    got = ba.read()
    for k in bp.EST:
        assert got[k].tobytes() == start[k].tobytes(), k
    flag.value = 0  # cleared: the same handle now does what a fresh one does
    st2 = _optimize(ctx, ba, 5, flag if kind == "int" else None)
    got2 = ba.read()
    ba.close()
    assert st2 == st_f and st2["iterations"] == 5
    for k in bp.EST:
        assert got2[k].tobytes() == res_f[k].tobytes(), k


# ----------------------------------------------------------------------------------------------- f. refusal
def test_pose_system_above_the_limit_is_refused(ctx):
    """667 free cameras and no edge: NP = 4002 > DYN_MAX_NP = 4000.  Refused before anything is allocated; *out stays NULL."""
    d = synth.ba_dyn_strip(synth.ba_dyn_problem(23, n_kf=6, n_points=10, n_objects=1, pts_per_obj=4), objects=False, dynamic=False, static=False)
    d["cam_pose"] = np.tile(d["cam_pose"][:1], (667, 1)); d["cam_fixed"] = np.zeros(667, np.uint8)
    assert bp.pose_offsets(d)[3] == 4002
    p = problem_struct(d)
    out = C.c_void_p()
    r = _lib.lib().cs_ba_dyn_create(ctx.ptr, C.byref(p), C.byref(out))
    assert _lib.STATUS[r] == "CS_ERR_BAD_ARG" and not out.value
    assert b"DYN_MAX_NP" in _lib.lib().cs_last_error(ctx.ptr)
    with pytest.raises(_lib.CubeSlamError, match="CS_ERR_BAD_ARG.*DYN_MAX_NP"):
        DynamicBundleAdjuster(d, ctx=ctx)
    d["cam_fixed"][0] = 1; d["vel"] = np.zeros((2, 2))  # 666 free cameras and two velocities: exactly 4000 scalars are accepted (no solve at this size)
    assert bp.pose_offsets(d)[3] == 4000
    ba = DynamicBundleAdjuster(d, ctx=ctx)
    ba.close()


def test_optimize_zero_iterations(ctx):
    d = bp.build("np64")
    ba = DynamicBundleAdjuster(d, ctx=ctx)
    start = ba.read()
    ctx.timing(True); ctx.timing_reset()
    try:
        st = ba.optimize(0)
        n = _counts(ctx)
    finally:
        ctx.timing(False)
    assert st == {"iterations": 0, "lm_trials": 0, "chi2_init": 0.0, "chi2_final": 0.0, "lambda_final": 0.0, "chi2_trace": []}
    assert sum(n.values()) == 0, n
    got = ba.read()
    ba.close()
    for k in bp.EST:
        assert got[k].tobytes() == start[k].tobytes(), k
