"""CPU: the preconditions of the Sim3Solver patterns (tests/sim3_solver_patterns.py), so that what the GPU tests and the pins compare is what they claim: a planted similarity
with inlier noise and gross outliers; the planted model's counts; no marginal correspondence in a deciding hypothesis of any pattern (marginal: err within the measured band
R.TOL_ERR around its threshold, where the reference's build and the stated definitions may decide differently; deciding: the hypotheses up to and including the first success,
all of them where there is none); at most 2 % of all hypotheses of a pattern with a marginal correspondence.  A seed that failed one of these was replaced; the cap is a
condition, not a measurement."""
import numpy as np
import pytest

from tests import sim3_solver_patterns as P
from tests import sim3_solver_restatement as R


def _planted_counts(c):
    """The inliers of the planted similarity itself (its float rounding as the hypothesis form: sR, t, sRinv, tinv)."""
    s, Rm, t = c["planted"]
    h = {"sR": (Rm.astype(np.float64) * float(s)).astype(np.float32).reshape(-1), "t": t,
         "sRinv": (Rm.T.astype(np.float64) / float(s)).astype(np.float32).reshape(-1)}
    h["tinv"] = (-(h["sRinv"].reshape(3, 3).astype(np.float64) @ t.astype(np.float64))).astype(np.float32)
    a, b = R.errors(h, c["X1"], c["X2"], c["K8"])
    return (a < c["e1"]) & (b < c["e2"])


@pytest.mark.parametrize("name", P.ALL)
def test_planted_model(name):
    c = P.solver_case(name)
    N = len(c["X1"])
    inl = _planted_counts(c)
    good = ~c["planted_outlier"]
    assert (c["e1"] == np.floor(c["e1"])).all() and c["e1"].min() >= 9  # float(size_t(9.210 * sigma2))
    assert inl[good].mean() >= 0.95 and inl[c["planted_outlier"]].sum() <= max(1, N // 50)  # the noise stays inside the thresholds, the outliers are gross
    assert len(np.unique(c["idx1"])) == N and c["idx1"].max() < c["mN1"] and c["mN1"] > N
    if name == "n15_too_few":
        assert c["max_its"] == 0
        return
    j = P.judged(name)
    assert len(j["n_inliers"]) == c["max_its"] and not np.isnan(j["sRt"]).any()
    first = P.first_success(name)
    if name in ("n100_no_consensus", "n20"):
        assert first == -1 and (name == "n20" or inl.sum() < P.MIN_INLIERS)  # (N == minInliers: one iteration whose count cannot exceed N)
    else:
        assert first >= 0 and j["n_inliers"].max() >= 0.9 * good.sum() and good.sum() > P.MIN_INLIERS


def test_seams_are_covered():
    sizes = sorted(len(P.solver_case(n)["X1"]) for n in P.ALL)
    assert {20, 21, 63, 64, 65, 129, 200} <= set(sizes)
    its = {n: P.solver_case(n)["max_its"] for n in P.ALL}
    assert its["n20"] == 1 and its["n15_too_few"] == 0 and its["n200"] == 300 and 1 < its["n21"] < 10 and any(P.solver_case(n)["fix_scale"] for n in P.ALL)


@pytest.mark.parametrize("name", [n for n in P.ALL if P.SOLVER_CASES[n][0] >= P.MIN_INLIERS])
def test_no_marginal_correspondence_where_it_decides(name):
    marg = P.margins(name)[0]
    H = len(marg)
    first = P.first_success(name)
    deciding = H if first < 0 else first + 1
    assert not marg[:deciding].any(), np.nonzero(marg[:deciding].any(1))[0]
    n_marginal = int(marg.any(1).sum())
    print("%s: %d of %d hypotheses hold a marginal correspondence" % (name, n_marginal, H))
    assert n_marginal <= 0.02 * H
