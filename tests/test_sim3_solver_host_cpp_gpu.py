"""GPU: the C++ mirror of Sim3Solver (cubeslam::Sim3Solver, cube_slam_amd/host/sim3_solver.hpp) compiled with g++ against the C-ABI library through
tests/cpp/sim3_solver_mirror.cpp: byte-equal to the Python mirror (cube_slam_amd/sim3_solver.py) on two sets of patterns -- the tables of evaluate_many (one device call for all
candidates), the scripted ComputeSim3 round-robin with rejected successes, and draw_triples."""
import os
import subprocess

import numpy as np
import pytest

from tests import sim3_solver_patterns as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("sim3_solver_mirror") / "sim3_solver_mirror")
    lib_dir = os.path.join(ROOT, "cube_slam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "sim3_solver_mirror.cpp"), "-o", e, "-L", lib_dir,
                           "-lcubeslam_hip", "-Wl,-rpath," + lib_dir])
    return e


@pytest.mark.parametrize("names,rejected", [(("n65", "n100_no_consensus", "n15_too_few", "n129"), ("n65",)), (("n20", "n64_fix", "n63", "n200", "n21"), ("n64_fix", "n63"))])
def test_cpp_mirror_equals_python_mirror(ctx, exe, tmp_path, names, rejected):
    from cube_slam_amd.sim3_solver import Sim3Solver
    names = list(names)
    reject = {(names.index(nm), P.first_success(nm)) for nm in rejected}
    c0 = P.solver_case(names[0])
    rng = np.random.RandomState(6)
    rnd = [int(rng.randint(0, len(c0["X1"]) - i)) for _ in range(c0["max_its"]) for i in range(3)]
    (tmp_path / "in.bin").write_bytes(P.mirror_input(names, reject, rnd))
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=60)

    solvers = []
    for nm in names:
        c = P.solver_case(nm)
        s = Sim3Solver(c["X1"], c["X2"], c["e1"], c["e2"], P.K1, P.K2, c["idx1"], c["mN1"], c["fix_scale"], ctx=ctx)
        s.SetRansacParameters(P.PROB, P.MIN_INLIERS, P.MAX_ITS)
        if s.mRansacMaxIts:
            s.set_triples(c["triples"])
        solvers.append(s)
    Sim3Solver.evaluate_many(solvers)
    tables = [s._table if s.mRansacMaxIts else None for s in solvers]
    log = P.round_robin(solvers, reject)
    assert sum(e[1] for e in log) >= 2  # a rejected success before the one that ends the loop
    it = iter(rnd)
    s0 = Sim3Solver(c0["X1"], c0["X2"], c0["e1"], c0["e2"], P.K1, P.K2, c0["idx1"], c0["mN1"], ctx=ctx)
    s0.SetRansacParameters(P.PROB, P.MIN_INLIERS, P.MAX_ITS)
    drawn = s0.draw_triples(lambda lo, hi: next(it))
    assert (tmp_path / "out.bin").read_bytes() == P.mirror_output(names, tables, log, drawn)
