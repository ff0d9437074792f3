"""GPU: the pose graph's sparse block Cholesky (eg_assemble, eg_factor over the level sets, eg_back of cube_slam_amd/csrc/posegraph.hip) through the probe
cs_essential_graph_solve (include/cubeslam_hip/essential_graph_solve.h), which issues the optimiser's own launches, against a dense solve of the same system on the designed
cases of tests/essential_graph_solve_patterns.py (their preconditions: tests/test_essential_graph_solve_patterns.py).

The judge is the backward error, with r = b - A x formed in long double: eta = |r|_2 / (|A|_2 |x|_2 + |b|_2), and the same per block row, |r_p|_2 against
|A_p,:|_2 |x|_2 + |b_p|_2, which names the vertex of a wrong block.  The tolerance is derived, not measured: eta <= 4 k u with u = 2^-53 and k = 7 * (longest row structure + 2),
the longest inner product the factor and the two substitutions form in the case (the row structure's blocks of 7, the diagonal block, the right-hand side), taken from the
symbolic analysis.  Higham's N (3 N + 1) u for a Cholesky solve, N = 7 nf, is the ceiling above it (printed) and is not used.  x is also held to the refined dense
solution within cond_2(A) * 4 k u of |x|_inf.  On the CPU a block Cholesky over the same structure that loses one update into one fill block has eta above 1e-7; 4 k u is
between 9e-15 and 1e-12.  Measured on the MI355X, 2026-10-21: eta 2.9e-18 .. 1.9e-16 over the 15 systems (LAPACK on the same: 2.7e-18 .. 1.2e-16), per block row at most 1.3e-16.

The failed solve is reached here too: a negative lambda, a zero pivot in a sequential chain, a NaN in J -- status 1, no x asserted, status 0 on the neighbouring good system."""
import ctypes as C

import numpy as np
import pytest

from cube_slam_amd import _lib
from cube_slam_amd import optimizer as O
from tests import essential_graph_solve_patterns as SP

gpu = pytest.mark.gpu
BAD_ARG = -2
CASES = [(name, lam) for name in SP.NAMES for lam in ((1e-16,) if name == "kf300_real" else SP.LAMBDAS)]


@pytest.fixture(scope="module")
def handles(ctx):
    """handles(name): one handle per case, made when first asked for and shared by the tests below; every one is closed when the module ends, before the context goes."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = O.EssentialGraph(SP.graph_dict(SP.make(name)), False, ctx=ctx)
        return made[name]

    yield get
    for eg in made.values():
        eg.close()


def _vertex_at(c, p):
    """The vertex whose column of L is at position p of the elimination order."""
    return c["sym"]["free"][c["sym"]["pos"].index(p)]


def _zeroed(c, v):
    """J with every Jacobian of vertex v zero: its diagonal block, its off-diagonal blocks and its b are zero."""
    J = c["J"].copy()
    J[c["ei"] == v, 0] = 0.0
    J[c["ej"] == v, 1] = 0.0
    return J


@gpu
@pytest.mark.parametrize("name,lam", CASES, ids=["%s-%g" % nl for nl in CASES])
def test_solve_against_the_dense_system(ctx, handles, name, lam):
    c, eg = SP.make(name), handles(name)
    s, k = SP.system(c, lam), SP.tolerance_k(c)
    bound = 4 * k * SP.U
    ctx.timing(True)
    ctx.timing_reset()
    x, status = eg.solve(c["J"], c["err"], lam)
    counts = [ctx.timing_get(kn)[1] for kn in ("eg_assemble", "eg_factor", "eg_back")]
    ctx.timing(False)
    xf = SP.free_rows(c, x)
    eta, per, at = SP.backward_errors(s, xf)
    ref = SP.backward_errors(s, s["x_lapack"])
    dx = float(np.max(np.abs(xf - s["x_ref"].astype(np.float64))) / np.max(np.abs(xf))) if np.all(np.isfinite(xf)) and np.any(xf) else np.inf
    print("%s lambda %g: status %d; eta %.3e (LAPACK %.3e), per block row %.3e at vertex %d (LAPACK %.3e); bound 4 k u = %.3e (k = %d), ceiling %.3e; x against the refined "
          "solution %.3e (cond %.3e, allowed %.3e); launches %s" % (name, lam, status, eta, ref[0], per, c["sym"]["free"][at], ref[1], bound, k, SP.higham_ceiling(c), dx, s["cond"], s["cond"] * bound, counts))
    assert status == 0
    assert x.shape == (c["n"], 7) and not x[c["fixed"]].any() and np.all(np.isfinite(x))
    assert eta <= bound and per <= bound
    assert dx <= s["cond"] * bound
    # the launches: one assembly, then as many factor and back-substitution launches as the Python analysis's launch list has entries.  Only the number is held: nothing
    # the library answers says which of them are parallel and which sequential
    n_launch = len(c["sym"]["launches"])
    assert counts == [1, n_launch, n_launch]
    # the same handle through the optimiser, then the probe again: the same bytes
    again = eg.solve(c["J"], c["err"], lam)
    assert again[0].tobytes() == x.tobytes() and again[1] == 0
    _, _, st = eg.optimize(c["Scw"], c["Snc"], c["has_nc"], iterations=1)
    assert st["launches_per_trial"] == 2 * n_launch + 3
    assert (st["levels"], st["l_blocks"], st["h_blocks"]) == (c["sym"]["levels"], c["sym"]["l_blocks"], c["sym"]["h_blocks"])
    third = eg.solve(c["J"], c["err"], lam)
    assert third[0].tobytes() == x.tobytes() and third[1] == 0


@gpu
def test_a_negative_lambda_fails_in_a_parallel_level_and_the_factor_still_runs(ctx, handles):
    c, eg = SP.make("grid6x6"), handles("grid6x6")
    assert c["sym"]["launches"][0][0] == "par" and float(np.max(np.diag(c["H"]))) < 1e3  # every first pivot is negative, in level 0 already
    good = eg.solve(c["J"], c["err"], 1e3)
    ctx.timing(True)
    ctx.timing_reset()
    x, status = eg.solve(c["J"], c["err"], -1e3)
    counts = [ctx.timing_get(kn)[1] for kn in ("eg_factor", "eg_back")]
    ctx.timing(False)
    print("grid6x6 lambda -1e3: status %d, %d of %d x finite, launches %s" % (status, int(np.isfinite(x).sum()), x.size, counts))
    assert status == 1 and counts == [len(c["sym"]["launches"])] * 2
    assert good[1] == 0
    after = eg.solve(c["J"], c["err"], 1e3)  # the status word is cleared by the next solve, and nothing of the failed one stays
    assert after[1] == 0 and after[0].tobytes() == good[0].tobytes()


@gpu
@pytest.mark.parametrize("position", [0, 15, 29])
def test_a_zero_pivot_in_a_sequential_chain(ctx, handles, position):
    """lambda = 0 with one free vertex's Jacobians zero: its diagonal block is zero when its turn comes -- the first column of path30's chain, a middle one, the root."""
    c, eg = SP.make("path30"), handles("path30")
    assert c["sym"]["launches"] == [("seq", 30)]
    v = _vertex_at(c, position)
    good = eg.solve(c["J"], c["err"], 0.0)
    x, status = eg.solve(_zeroed(c, v), c["err"], 0.0)
    print("path30 lambda 0, vertex %d (position %d) zeroed: status %d, %d of %d x finite" % (v, position, status, int(np.isfinite(x).sum()), x.size))
    assert status == 1 and good[1] == 0
    s = SP.system(c, 1e-16)  # the neighbouring good system: lambda = 0 is below half a unit of every diagonal entry, so A is the same matrix
    assert SP.with_lambda(c["H"], 0.0).tobytes() == s["A"].tobytes()
    eta = SP.backward_errors(s, SP.free_rows(c, good[0]))
    assert max(eta[:2]) <= 4 * SP.tolerance_k(c) * SP.U


@gpu
@pytest.mark.parametrize("name", ["multi", "grid6x6"])
def test_one_nan_in_j_fails_the_solve(ctx, handles, name):
    c, eg = SP.make(name), handles(name)
    e = len(c["ei"]) // 2
    side = 0 if int(c["ei"][e]) != c["fixed"] else 1
    J = c["J"].copy()
    J[e, side, 3, 4] = np.nan
    x, status = eg.solve(J, c["err"], 1.0)
    print("%s, one NaN in J: status %d, %d of %d x finite" % (name, status, int(np.isfinite(x).sum()), x.size))
    assert status == 1
    good = eg.solve(c["J"], c["err"], 1.0)
    assert good[1] == 0 and np.all(np.isfinite(good[0]))
    # a NaN on the fixed vertex's side is not read at all
    ef = int(np.flatnonzero((c["ei"] == c["fixed"]) | (c["ej"] == c["fixed"]))[0])
    J = c["J"].copy()
    J[ef, 0 if int(c["ei"][ef]) == c["fixed"] else 1] = np.nan
    unread = eg.solve(J, c["err"], 1.0)
    assert unread[1] == 0 and unread[0].tobytes() == good[0].tobytes()


@gpu
def test_a_non_finite_lambda_is_not_an_error(ctx, handles):
    c, eg = SP.make("multi"), handles("multi")
    x, status = eg.solve(c["J"], c["err"], float("nan"))
    assert status == 1  # NaN > 0 is false on the first pivot
    x, status = eg.solve(c["J"], c["err"], float("inf"))
    # an infinite diagonal: every pivot is inf > 0, every entry below a pivot and every substitution is a finite number over inf, and inf is only ever a divisor
    assert status == 0 and not x.any()
    assert eg.solve(c["J"], c["err"], 1.0)[1] == 0


@gpu
def test_bad_arguments_are_errors_and_launch_nothing(ctx, handles):
    c, eg = SP.make("multi"), handles("multi")
    J, err, x, st = np.ascontiguousarray(c["J"]).reshape(-1, 14, 7), c["err"], np.full((c["n"], 7), 7.0), C.c_int(5)
    ptr, call = _lib.ptr, _lib.lib().cs_essential_graph_solve
    other = _lib.Context(0)
    try:
        ctx.timing(True)
        ctx.timing_reset()
        other.timing(True)
        other.timing_reset()
        assert call(other.ptr, eg._h, ptr(J), ptr(err), 1.0, ptr(x), C.byref(st)) == BAD_ARG  # a handle of another context
        assert call(None, eg._h, ptr(J), ptr(err), 1.0, ptr(x), C.byref(st)) == BAD_ARG
        assert call(ctx.ptr, None, ptr(J), ptr(err), 1.0, ptr(x), C.byref(st)) == BAD_ARG
        assert call(ctx.ptr, eg._h, None, ptr(err), 1.0, ptr(x), C.byref(st)) == BAD_ARG
        assert call(ctx.ptr, eg._h, ptr(J), None, 1.0, ptr(x), C.byref(st)) == BAD_ARG
        assert call(ctx.ptr, eg._h, ptr(J), ptr(err), 1.0, None, C.byref(st)) == BAD_ARG
        assert call(ctx.ptr, eg._h, ptr(J), ptr(err), 1.0, ptr(x), None) == BAD_ARG
        for k in ("eg_assemble", "eg_factor", "eg_back"):
            assert ctx.timing_get(k)[1] == 0 and other.timing_get(k)[1] == 0
        assert st.value == 5 and (x == 7.0).all()
        ctx.timing(False)
    finally:
        other.close()
    with pytest.raises(ValueError):
        eg.solve(c["J"][:-1], c["err"], 1.0)
    with pytest.raises(ValueError):
        eg.solve(c["J"], c["err"][:-1], 1.0)
    assert eg.solve(c["J"], c["err"], 1.0)[1] == 0  # the handle is usable afterwards
