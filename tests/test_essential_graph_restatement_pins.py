"""The judge of the pose graph's GPU tests (tests/essential_graph_restatement.py) against the reference's own text: Optimizer::OptimizeEssentialGraph
(orb_object_slam/src/Optimizer.cc:2575-2836) is cut out of the reference at test time into tmp_path, compiled there around tests/cpp/ref_essential_graph_standins.cpp (our stand-ins
for KeyFrame / MapPoint / Map / LoopClosing / Converter) exactly as tests/sim3_opt_restatement.py::build_reference compiles OptimizeSim3, and run on the cases of
tests/essential_graph_patterns.py.  The edge list must be equal entry for entry; estimates, float poses and corrected points must agree within R.TOL_* = 10 x D_REF_*, where D_REF_* is
how far the reference's own output moves when the order of its key frames is permuted, measured here.  The reference's linear solver in this build is the dense shadow of
linear_solver_eigen.h, not Eigen's sparse Cholesky: nothing beyond the edge list is expected to be equal bit for bit, and nothing is claimed to be.  That solver takes 140 s on the
300-vertex case, which is therefore left to the GPU test and the bench tool.  Nothing cut or compiled is written inside the repository."""
import numpy as np
import pytest

from tests import essential_graph_patterns as P
from tests import essential_graph_restatement as R

pytestmark = pytest.mark.skipif(not R.reference_available(), reason="needs the reference under /root/reference and the g2o objects build() makes in oracle/_ref")
PIN_CASES = [k for k in P.CASES if k != "kf300"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build_reference(tmp_path_factory.mktemp("ref_essential_graph"))


def _by_id(mp, res):
    o = np.argsort([kf.mnId for kf in mp.all_kfs])
    return res["sim3"][o], res["Tiw"][o], res["points"]


@pytest.mark.parametrize("name", PIN_CASES)
def test_restatement_equals_the_reference(ref, name):
    mp, fix, j = P.case(name), P.CASES[name][1], P.judged(name)
    r = R.run_reference(ref, mp, fix)
    ids = np.array([kf.mnId for kf in mp.all_kfs])
    ei, ej, _ = j["edges"]
    assert np.array_equal(np.stack([ids[ei], ids[ej]], axis=1), r["edges"])  # the edges the reference hands to addEdge, in its order
    d = (R.sim3_distance(j["sim3"], r["sim3"]), R.abs_distance(j["Tiw"], r["Tiw"]), R.abs_distance(j["points"], r["points"]))
    print("%s: %d edges; trials per iteration %s / %s; sim3 %.3e (TOL %.3e), Tiw %.3e (TOL %.3e), points %.3e (TOL %.3e); reference %.4f s"
          % (name, len(ei), R.per_iteration(j["stats"]["sequence"]), r["trials_per_iteration"], d[0], R.TOL_SIM3, d[1], R.TOL_TIW, d[2], R.TOL_POINTS, r["seconds"]))
    assert R.per_iteration(j["stats"]["sequence"]) == r["trials_per_iteration"]  # what g2o prints per iteration: levenbergIter
    assert d[0] <= R.TOL_SIM3 and d[1] <= R.TOL_TIW and d[2] <= R.TOL_POINTS


def test_reference_order_sensitivity(ref):
    """D_REF_*: five seeded permutations of GetAllKeyFrames() (and with it of the addresses that order every std::set) per case.  The trials per iteration must not move at all."""
    worst = [0.0, 0.0, 0.0]
    for name in PIN_CASES:
        mp, fix = P.case(name), P.CASES[name][1]
        r0 = R.run_reference(ref, mp, fix)
        a = _by_id(mp, r0)
        w = [0.0, 0.0, 0.0]
        for s in range(5):
            m2 = mp.permuted(np.random.RandomState(100 + s).permutation(len(mp.all_kfs)))
            r = R.run_reference(ref, m2, fix)
            b = _by_id(m2, r)
            assert r["trials_per_iteration"] == r0["trials_per_iteration"], name
            w = [max(x, y) for x, y in zip(w, (R.sim3_distance(b[0], a[0]), R.abs_distance(b[1], a[1]), R.abs_distance(b[2], a[2])))]
        print("%s: sim3 %.3e Tiw %.3e points %.3e" % ((name,) + tuple(w)))
        worst = [max(x, y) for x, y in zip(worst, w)]
    print("D_REF_SIM3 = %r, D_REF_TIW = %r, D_REF_POINTS = %r" % tuple(worst))
    for got, const in zip(worst, (R.D_REF_SIM3, R.D_REF_TIW, R.D_REF_POINTS)):
        assert 0.5 * const <= got <= const
    assert (R.TOL_SIM3, R.TOL_TIW, R.TOL_POINTS) == (10 * R.D_REF_SIM3, 10 * R.D_REF_TIW, 10 * R.D_REF_POINTS)
