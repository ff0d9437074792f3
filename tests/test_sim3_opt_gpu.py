"""GPU parity: the batched Sim3 refinement (cs_sim3_optimization, one workgroup per problem) through the C-ABI against the restatement of Optimizer::OptimizeSim3
(tests/sim3_opt_restatement.py, pinned to the reference's own text by tests/test_sim3_opt_restatement_pins.py).  The return value and the removed flags must be equal in
every case (tests/test_sim3_opt_patterns.py shows that no chi2 sits on the threshold); the Sim3 must agree within R.TOL = 10 x D_REF, the reference's own sensitivity to
the order of its correspondences."""
import os
import re

import numpy as np
import pytest

from cube_slam_amd import _lib
from cube_slam_amd.optimizer import OptimizeSim3
from tests import sim3_opt_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu


def test_the_library_exports_the_entry_and_the_header_declares_it():
    assert hasattr(_lib.lib(), "cs_sim3_optimization")
    header = open(os.path.join(ROOT, "include", "cubeslam_hip.h")).read()
    assert re.search(r"\bint\s+cs_sim3_optimization\s*\(\s*cs_ctx\s*\*\s*ctx\s*,\s*int\s+n_problems\s*,", header)
    assert "Optimizer::OptimizeSim3" in header and "Optimizer.cc:2838-3033" in header and _lib.header_version() == 108


def _check(name, got):
    c = R.case(name)
    pose, removed, n_in = got
    wpose, wremoved, wn, st = R.judged(name)
    d = R.pose_distance(pose, wpose)
    print("%s: n_inliers %d / %d, flags differing %d, distance %.3e (TOL %.3e)" % (name, n_in, wn, int((removed != wremoved).sum()), d, R.TOL))
    assert n_in == wn
    assert np.array_equal(removed, wremoved)
    assert d <= R.TOL
    if st["early"]:
        assert pose.tobytes() == np.ascontiguousarray(c["sim3_in"], np.float64).tobytes()


@gpu
@pytest.mark.parametrize("name", list(R.CASES))
def test_device_equals_the_restatement(ctx, name):
    got = OptimizeSim3(R.case(name), ctx=ctx)
    _check(name, got)
    c = R.case(name)
    if name == "n12_3out":  # returns 0, the pose untouched, exactly the three gross outliers flagged
        assert got[2] == 0 and np.array_equal(np.nonzero(got[1])[0], c["outliers"]) and len(c["outliers"]) == 3
    if name == "fix_scale_on":
        assert got[2] > 0 and got[0][7] == c["sim3_in"][7] and got[0].tobytes() != c["sim3_in"].tobytes()  # s leaves exactly as it came, the rest moved
    if name == "fix_scale_off":
        assert got[0][7] != c["sim3_in"][7]


@gpu
def test_a_batch_equals_its_problems_alone_and_itself(ctx):
    problems = [R.case(k) for k in R.BATCH]
    batch = OptimizeSim3(problems, ctx=ctx)
    again = OptimizeSim3(problems, ctx=ctx)
    assert len(batch) == 7
    for k, b, a in zip(R.BATCH, batch, again):
        s = OptimizeSim3(R.case(k), ctx=ctx)
        assert b[0].tobytes() == s[0].tobytes() == a[0].tobytes() and b[1].tobytes() == s[1].tobytes() == a[1].tobytes() and b[2] == s[2] == a[2], k
        _check(k, b)
    back = OptimizeSim3(problems[::-1], ctx=ctx)[::-1]  # a problem's result does not depend on its place or its neighbours
    for b, r in zip(batch, back):
        assert b[0].tobytes() == r[0].tobytes() and b[1].tobytes() == r[1].tobytes() and b[2] == r[2]


@gpu
def test_bad_arguments_are_errors(ctx):
    c = dict(R.case("n10"))
    c["obs1"] = c["obs1"][:-1]
    with pytest.raises(ValueError):
        OptimizeSim3(c, ctx=ctx)
    assert OptimizeSim3([], ctx=ctx) == []
