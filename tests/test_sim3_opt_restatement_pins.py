"""The judge of the Sim3 refinement's GPU tests (tests/sim3_opt_restatement.py) against the reference's own text: Optimizer::OptimizeSim3 (orb_object_slam/src/Optimizer.cc:2838-3033)
is cut out of the reference at test time into tmp_path, compiled there around tests/cpp/ref_sim3_opt_standins.cpp (our stand-ins for KeyFrame / MapPoint / Converter;
oracle/ref_shim/cvshim.hpp for cv::Mat, oracle/ref_shim/eigen_full for Eigen) with the reference's types_seven_dof_expmap.cpp, linked with the g2o core / types / stuff objects that
build() leaves in oracle/_ref, and run on every case of tests/test_sim3_opt_gpu.py.  The return value and the removed flags must be equal; the eight numbers of the Sim3 must agree
within R.TOL = 10 x D_REF, where D_REF is the reference's own sensitivity to the order of its correspondences, measured here.  Nothing cut or compiled is written inside the
repository."""
import numpy as np
import pytest

from tests import sim3_opt_restatement as R

pytestmark = pytest.mark.skipif(not R.reference_available(), reason="needs the reference under /root/reference and the g2o objects build() makes in oracle/_ref")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return R.build_reference(tmp_path_factory.mktemp("ref_sim3_opt"))


def test_cut_takes_the_whole_definition():
    text = "int f(int a)\n{\n  if (a) { return 1; }\n  return 0;\n}\nint g() { return 2; }\n"
    assert R._cut(text, "int f(int a)") == "int f(int a)\n{\n  if (a) { return 1; }\n  return 0;\n}" and R._cut(text, "int g()") == "int g() { return 2; }"


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_equals_the_reference(ref, name):
    c = R.case(name)
    pose, removed, n_in, _ = R.judged(name)
    rpose, rremoved, rn = R.run_reference(ref, c)
    d = R.pose_distance(pose, rpose)
    print("%s: n_inliers %d / %d, distance %.3e (TOL %.3e)" % (name, n_in, rn, d, R.TOL))
    assert n_in == rn and np.array_equal(removed, rremoved)
    assert d <= R.TOL
    if n_in == 0:
        assert rpose.tobytes() == np.ascontiguousarray(c["sim3_in"], np.float64).tobytes()  # g2oS12 is not written on the early return


def test_reference_order_sensitivity(ref):
    """D_REF: how far the reference's own output moves when only the order of its correspondences is reversed; flags and return value do not move at all."""
    worst = 0.0
    for name in R.CASES:
        c = R.case(name)
        n = len(c["inv_sigma2_1"])
        a, fa, na = R.run_reference(ref, c)
        b, fb, nb = R.run_reference(ref, c, order=np.arange(n)[::-1])
        d = R.pose_distance(b, a)
        print("%s: %.3e" % (name, d))
        assert na == nb and np.array_equal(fa, fb)
        worst = max(worst, d)
    print("D_ref = %r" % worst)
    assert 0.5 * R.D_REF <= worst <= R.D_REF and R.TOL == 10 * R.D_REF
