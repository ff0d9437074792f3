"""GPU parity of the Sim3 refinement (sim3_opt_kernel, cs_sim3_optimization) on the way it takes, not only where it ends: per Levenberg-Marquardt trial, at the exits,
under both stage-two budgets and in batches whose problems differ in th2, K and fix_scale -- through the probes of include/cubeslam_hip/sim3_opt_trace.h against the
restatement (tests/sim3_opt_restatement.py, pinned to the reference's own text by tests/test_sim3_opt_restatement_pins.py).  tests/test_sim3_opt_patterns.py shows on the
CPU that every case takes the path it claims, that the tolerances are ten times what reordering the correspondences does to the restatement itself, and that each of three
bugs the end pose forgives (rho[1] missing in H, lambda0 ten times too large, a rejected trial not undone) is 100 times outside them.

What is asked: n_inliers and flags equal, the pose within R.TOL (as tests/test_sim3_opt_gpu.py asks of every case, the new ones included); the probe's three outputs
byte-equal to the product's; system0 within R.SYS0_TOL; on each case's decisive prefix stage, iteration, solved and accepted equal, currentChi / tempChi / lambda within
ten times that trial's own order figure; cs_sim3_exp within ten times each update's float64-to-longdouble distance.

Observed on an MI355X (each test prints its figures; DESIGN.md 7.10 has them by case): flags, counts and the probe's bytes equal everywhere; the new cases' poses 3.6e-14
(exact) to 6.1e-07 (budget10) from the restatement (R.TOL 4.8e-06); system0 at most 2.1e-15 (n2000; R.SYS0_TOL 4.2e-14); on the decisive prefixes (2 to 22 trials) stage,
iteration, solved and accepted equal in all 32 cases, chi2 at most 0.34 of its trial's tolerance (behind, trial 8; the largest difference itself is 2.1e-03, a rejected
trial's tempChi in budget10) and lambda at most 0.16 (budget10; 1.2e-06 in budget5); cs_sim3_exp at most 1.7e-16 from the restatement, 669 of 729 rows equal to the bit.
Beyond the prefixes the ways part as expected (n11 runs 20 trials where the restatement runs 18, fix_clean 7 where it runs 27) and only the ends are compared."""
import numpy as np
import pytest

from cube_slam_amd import _lib
from cube_slam_amd.optimizer import OptimizeSim3, OptimizeSim3Trace, sim3_exp
from tests import sim3_opt_restatement as R
from tests.test_sim3_opt_gpu import _check

pytestmark = pytest.mark.gpu

BAD_ARG = -2  # CS_ERR_BAD_ARG
_runs = {}


def _traced(ctx, name):
    """The probe's result for a case, computed once."""
    if name not in _runs:
        _runs[name] = OptimizeSim3Trace(R.case(name), R.MAX_TRIALS, ctx=ctx)
    return _runs[name]


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


@pytest.mark.parametrize("name", R.NEW_CASES)
def test_new_case_alone_equals_the_restatement(ctx, name):
    c = R.case(name)
    got = OptimizeSim3(c, ctx=ctx)
    _check(name, got)
    pose, removed, n_in = got
    sim3_in = np.ascontiguousarray(c["sim3_in"], np.float64)
    assert np.isfinite(pose).all()
    if name in ("zero_weights", "all_outliers"):  # twenty failed solves, or the early return: the pose leaves bit for bit as it came
        assert pose.tobytes() == sim3_in.tobytes()
    if name == "zero_weights":
        assert n_in == len(removed) == 40 and not removed.any()
    if name == "all_outliers":
        assert n_in == 0 and removed.all()
    if name == "n13_3out":
        assert n_in == 10 and np.array_equal(np.nonzero(removed)[0], c["outliers"]) and pose.tobytes() != sim3_in.tobytes()
    if name == "behind":
        assert removed[R.CASES[name][0]["behind"][0]] == 1
    if name in ("fix_clean", "fix_a"):
        assert pose[7] == sim3_in[7] and pose.tobytes() != sim3_in.tobytes()
    if name == "fix_b":
        assert pose[7] != sim3_in[7]
    if name in ("budget10", "budget5"):  # the other budget's end, by the restatement, is not this one
        other = R.optimize_sim3(c, stage2_budget=5 if name == "budget10" else 10)
        assert R.pose_distance(pose, other[0]) > 99 * R.TOL or not np.array_equal(removed, other[1])


def test_removed_sets_differ_under_the_three_thresholds(ctx):
    a, b, c = (OptimizeSim3(R.case(k), ctx=ctx)[1] for k in ("th2_5.991", "th2_7.815", "th2_20"))
    assert not np.array_equal(a, b) and not np.array_equal(b, c) and not np.array_equal(a, c)
    ka, kb = OptimizeSim3(R.case("k_a"), ctx=ctx)[0], OptimizeSim3(R.case("k_b"), ctx=ctx)[0]
    assert R.pose_distance(ka, kb) > 1000 * R.TOL


def test_the_probe_equals_the_product(ctx):
    """cs_sim3_optimization_trace launches the product's kernel: the three outputs are byte-equal, alone and in a batch, whatever max_trials is."""
    names = list(R.BATCH) + list(R.NEW_CASES)
    problems = [R.case(k) for k in names]
    product = OptimizeSim3(problems, ctx=ctx)
    probe = OptimizeSim3Trace(problems, R.MAX_TRIALS, ctx=ctx)
    for k, a, b in zip(names, product, probe):
        assert _same(a, b), k
        alone = _traced(ctx, k)
        assert _same(a, alone) and np.array_equal(b[3], alone[3]) and b[4] == alone[4] and np.array_equal(b[5], alone[5]), k  # the trace does not depend on the neighbours
        want = R.judged(k)[3]
        assert b[4] == len(b[3]) <= R.MAX_TRIALS and (b[4] > 0) == (len(want["trace"]) > 0)
    # trials beyond max_trials are counted and not stored; none at all is allowed
    short = OptimizeSim3Trace(problems, 3, ctx=ctx)
    none = OptimizeSim3Trace(problems, 0, ctx=ctx)
    for k, a, s, z in zip(names, probe, short, none):
        assert _same(a, s) and _same(a, z) and s[4] == z[4] == a[4], k
        assert np.array_equal(s[3], a[3][:3]) and len(z[3]) == 0 and np.array_equal(s[5], a[5]) and np.array_equal(z[5], a[5]), k
    n0 = probe[names.index("n0")]
    assert n0[4] == 0 and len(n0[3]) == 0 and not n0[5].any()


@pytest.mark.parametrize("name", R.TRACED)
def test_first_system_and_decisive_trials_equal_the_restatement(ctx, name):
    """Observed on an MI355X: system0 1.2e-16 (exact) to 2.1e-15 (n2000); chi2 within 0.02 (stride_m1) to 0.34 (behind) of the trial's tolerance, lambda within 0.16
    (budget10); zero_weights equal to the bit over all twenty records.  The figure of a trial is the largest over four reorderings of the restatement: with the reversal alone
    outliers_10_more stood at 2.3 times its tolerance at one rejected trial, the scatter of a single draw and not a difference of the kernel."""
    pose, removed, n_in, trace, n_trials, system0 = _traced(ctx, name)
    want = R.judged(name)[3]
    w = R.compare_way(name, system0, trace)
    print("%s: system0 %.3e (tol %.3e); prefix %d of %d / %d trials: structure %s, chi %.3e (%.3f of its tolerance, at trial %d), lambda %.3e (%.3f of its tolerance)"
          % (name, w["sys0"], R.SYS0_TOL, w["prefix"], len(want["trace"]), n_trials, "equal" if w["same"] else "DIFFERS", w["chi"], w["chi_ratio"], w["chi_trial"], w["lambda"], w["lambda_ratio"]))
    assert np.isfinite(trace).all() and np.isfinite(system0).all() and n_trials == len(trace)
    assert w["sys0"] <= R.SYS0_TOL
    assert w["same"]
    assert w["chi_ratio"] <= 1.0 and w["lambda_ratio"] <= 1.0
    assert set(np.unique(trace[:, 0])) <= {0.0, 1.0} and set(np.unique(trace[:, 5])) <= {0.0, 1.0} and set(np.unique(trace[:, 6])) <= {0.0, 1.0}
    if name == "zero_weights":  # H = 0, lambda0 = 0: the whole trace is exact
        assert np.array_equal(trace, want["trace"]) and not system0.any()
    if name in ("budget10", "budget5"):  # the budget itself: iterations entered in stage two
        its = len(np.unique(trace[trace[:, 0] == 1][:, 1]))
        assert its == want["stage_iterations"][1] and (its >= 6 if name == "budget10" else its == 5)


@pytest.mark.parametrize("pair", R.PAIRS)
def test_each_problem_reads_its_own_parameters(ctx, pair):
    """One geometry under two th2, two K2 or with and without fix_scale, side by side: a kernel that read problem 0's parameter for both would fail one of them."""
    alone = [OptimizeSim3(R.case(k), ctx=ctx) for k in pair]
    assert not _same(alone[0], alone[1])
    for order in ((0, 1), (1, 0)):
        batch = OptimizeSim3([R.case(pair[i]) for i in order], ctx=ctx)
        for got, i in zip(batch, order):
            assert _same(got, alone[i]), (pair[i], order)
            _check(pair[i], got)


def test_sim3_exp_equals_the_restatement(ctx):
    """cs_sim3_exp on R.EXP_UPDATES: the four branches at eps, one ulp either side, the quaternion's second branch near pi, the zero update."""
    want, d, tol = R.exp_judged()
    got = sim3_exp(R.EXP_UPDATES, ctx=ctx)
    assert got.shape == want.shape and np.isfinite(got).all()
    assert got[0].tobytes() == want[0].tobytes()  # exp(0) is the identity, exactly
    dist = np.array([R.pose_distance(g, w) for g, w in zip(got, want)])
    worst = int(np.argmax(dist / tol))
    print("cs_sim3_exp: largest distance %.3e (R.EXP_TOL %.3e); largest share of a row's own tolerance %.3f, at update %s (distance %.3e, tolerance %.3e); rows equal to the bit %d of %d"
          % (dist.max(), R.EXP_TOL, (dist / tol).max(), R.EXP_UPDATES[worst].tolist(), dist[worst], tol[worst], int((got == want).all(axis=1).sum()), len(got)))
    assert (np.sign(got[:, 3:7]) == np.sign(want[:, 3:7]))[-8:].all()  # the written-out cases put each component where Eigen puts it, sign included
    assert (dist <= tol).all()


def test_bad_arguments_are_refused_before_the_device(ctx):
    """Through the C entries themselves: each refusal returns CS_ERR_BAD_ARG and leaves sim3_out, removed, n_inliers (and the probe's three arrays) as they were."""
    names = ("n11", "n13_3out")
    cs = [R.case(k) for k in names]
    off = np.array([0, 11, 24], np.int32)
    cat = lambda k, w: np.ascontiguousarray(np.concatenate([np.asarray(c[k], np.float64).reshape(-1, w) for c in cs]))
    arr = {"P1c": cat("P1c", 3), "P2c": cat("P2c", 3), "obs1": cat("obs1", 2), "obs2": cat("obs2", 2), "inv_sigma2_1": cat("inv_sigma2_1", 1), "inv_sigma2_2": cat("inv_sigma2_2", 1),
           "intrinsics": np.ascontiguousarray(np.stack([c["intrinsics"] for c in cs])), "sim3_in": np.ascontiguousarray(np.stack([c["sim3_in"] for c in cs]))}
    th2, fix = np.array([c["th2"] for c in cs], np.float32), np.array([c["fix_scale"] for c in cs], np.uint8)
    sout, flags, ninl = np.full((2, 8), 77.0), np.full(24, 7, np.uint8), np.full(2, -7, np.int32)
    trace, ntr, sys0 = np.full((2, 8, 7), 77.0), np.full(2, -7, np.int32), np.full((2, 36), 77.0)
    ptr = _lib.ptr
    good = {"n_problems": 2, "corr_off": ptr(off)}
    good.update({k: ptr(v) for k, v in arr.items()})
    good.update({"th2": ptr(th2), "fix_scale": ptr(fix), "sim3_out": ptr(sout), "removed": ptr(flags), "n_inliers": ptr(ninl)})
    order = ("n_problems", "corr_off", "P1c", "P2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "intrinsics", "sim3_in", "th2", "fix_scale", "sim3_out", "removed", "n_inliers")
    extra = {"max_trials": 8, "trace": ptr(trace), "n_trials": ptr(ntr), "system0": ptr(sys0)}

    def product(**kw):
        a = dict(good, **kw)
        return _lib.lib().cs_sim3_optimization(ctx.ptr, *[a[k] for k in order])

    def probe(**kw):
        a = dict(good, **dict(extra, **kw))
        return _lib.lib().cs_sim3_optimization_trace(ctx.ptr, *[a[k] for k in order], a["max_trials"], a["trace"], a["n_trials"], a["system0"])

    def untouched():
        return bool(np.all(sout == 77.0) and np.all(flags == 7) and np.all(ninl == -7) and np.all(trace == 77.0) and np.all(ntr == -7) and np.all(sys0 == 77.0))

    for call in (product, probe):
        for bad in ([0, 11, 10], [0, 24, 0], [5, 3, 24], [1, 11, 24], [3, 14, 27], [-1, 11, 24]):  # decreasing offsets; offsets that do not start at 0
            d = np.array(bad, np.int32)
            assert call(corr_off=ptr(d)) == BAD_ARG and untouched(), bad
        for k in order[1:]:
            assert call(**{k: None}) == BAD_ARG and untouched(), k
        assert call(n_problems=-1) == BAD_ARG and untouched()
        assert call(n_problems=0) == _lib.CS_OK and untouched()
    for k in ("trace", "n_trials", "system0"):
        assert probe(**{k: None}) == BAD_ARG and untouched(), k
    assert probe(max_trials=-1) == BAD_ARG and untouched()
    assert _lib.lib().cs_sim3_optimization(None, *[good[k] for k in order]) == BAD_ARG and untouched()
    assert product(n_problems=0, **{k: None for k in order[1:]}) == _lib.CS_OK and untouched()
    assert probe(n_problems=0, trace=None, n_trials=None, system0=None, **{k: None for k in order[1:]}) == _lib.CS_OK and untouched()
    assert probe(max_trials=0, trace=None) == _lib.CS_OK and np.all(trace == 77.0) and not np.any(sys0 == 77.0) and np.all(ntr > 0)  # no record asked for, none needed
    u, o = np.zeros((2, 7)), np.full((2, 8), 77.0)
    for r in (_lib.lib().cs_sim3_exp(ctx.ptr, -1, ptr(u), ptr(o)), _lib.lib().cs_sim3_exp(ctx.ptr, 2, None, ptr(o)), _lib.lib().cs_sim3_exp(ctx.ptr, 2, ptr(u), None)):
        assert r == BAD_ARG and np.all(o == 77.0)
    assert _lib.lib().cs_sim3_exp(ctx.ptr, 0, None, None) == _lib.CS_OK
    # and the arrays are good ones: the same calls go through, write every result and equal the runs alone
    sout[:], flags[:], ninl[:] = 77.0, 7, -7
    assert product() == _lib.CS_OK and not np.any(sout == 77.0) and np.all(flags <= 1) and np.all(ninl >= 0)
    first = (sout.copy(), flags.copy(), ninl.copy())
    assert probe() == _lib.CS_OK and np.array_equal(sout, first[0]) and np.array_equal(flags, first[1]) and np.array_equal(ninl, first[2])
    for i, k in enumerate(names):
        alone = _traced(ctx, k)
        assert _same((sout[i], flags[off[i]:off[i + 1]], int(ninl[i])), alone), k
        assert ntr[i] == alone[4] and np.array_equal(trace[i][:min(8, ntr[i])], alone[3][:8]) and np.array_equal(sys0[i], alone[5]), k
    assert OptimizeSim3Trace([], ctx=ctx) == []
