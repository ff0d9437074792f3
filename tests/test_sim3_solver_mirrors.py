"""CPU: (1) the two host-only rules of the library -- cs_sim3_solver_walk and cs_sim3_solver_max_iterations -- and draw_triples against the literal Python transcription of
Sim3Solver::iterate / SetRansacParameters (orb_object_slam/src/Sim3Solver.cc:112-205, tests/sim3_solver_restatement.py) over random tables of counts; (2) the HD text the
kernel runs (cube_slam_amd/csrc/horn_math.h) under the one host statement of a hypothesis (csrc/sim3_host.h), compiled by g++ into the C++ mirror's host path
(tests/cpp/sim3_solver_mirror.cpp `host`, built with nothing of the library, plain and with -fsanitize=address,undefined) and by the library's host compiler into the Python
mirror's (ctx=None), give the restatement's tables bit for bit on every pattern, and both mirrors walk the scripted round-robin alike."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import sim3_solver_patterns as P
from tests import sim3_solver_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP = C.POINTER(C.c_int)


def test_symbols_and_declarations():
    import cube_slam_amd
    from cube_slam_amd import _lib
    assert hasattr(cube_slam_amd, "Sim3Solver")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cubeslam_hip.h")).read(), flags=re.S)
    for name in ("cs_sim3_solver_hypotheses", "cs_sim3_solver_mask_words", "cs_sim3_solver_max_iterations", "cs_sim3_solver_walk"):
        assert hasattr(_lib.lib(), name), name
        assert re.search(r"\b%s\s*\(" % name, header), name


def _walk_both(counts, N, min_inliers, max_its, schedule, reject=()):
    """The library's walk and the transcription over one table with the iterate(n) calls of `schedule` -> both logs."""
    from cube_slam_amd._lib import lib
    counts = np.ascontiguousarray(counts, np.int32)
    tr = R.IterateTranscription(N, N, list(range(N)), min_inliers, max_its)
    it, best, hyp, nomore = C.c_int(0), C.c_int(0), C.c_int(-1), C.c_int(0)
    a, b = [], []
    for n in schedule:
        h, nm, _, nin = tr.iterate(n, counts)
        a.append((h, bool(nm), nin, tr.mnIterations, tr.mnBestInliers, tr.best))
        if N < min_inliers:  # :144 is the mirror's
            b.append((-1, True, 0, 0, 0, -1))
            continue
        t = lib().cs_sim3_solver_walk(counts.ctypes.data_as(IP), max_its, min_inliers, C.byref(it), C.byref(best), C.byref(hyp), n, C.byref(nomore))
        b.append((t, bool(nomore.value), int(counts[t]) if t >= 0 else 0, it.value, best.value, hyp.value))
    return a, b


def test_walk_random_tables():
    rng = np.random.RandomState(5)
    for _ in range(300):
        max_its = int(rng.randint(1, 40)); min_inl = int(rng.randint(3, 12))
        counts = rng.randint(0, 2 * min_inl + 2, max_its)
        if rng.rand() < 0.5:
            counts = np.minimum(counts, min_inl + (rng.rand(max_its) < 0.1))  # mostly no success, a few just above: ties with the best
        schedule = [int(rng.choice([1, 2, 5, 7, 50])) for _ in range(int(rng.randint(1, 12)))]
        a, b = _walk_both(counts, 60, min_inl, max_its, schedule)
        assert a == b, (counts, schedule)


def test_walk_named_tables():
    m = 20
    # ties with the best: the later hypothesis becomes the best (>=), but only a count above minInliers succeeds
    a, b = _walk_both([7, 7, 7, 3, 7], 60, m, 5, [2, 2, 2])
    assert a == b and [e[5] for e in a] == [1, 2, 4] and all(e[0] == -1 for e in a) and a[-1][1]
    # a success rejected by the caller, then a smaller success-sized count: it must not succeed (25 < mnBestInliers = 30); the equal one later does
    a, b = _walk_both([30, 25, 25, 30, 2], 60, m, 5, [5, 5, 5])
    assert a == b and [e[0] for e in a] == [0, 3, -1] and a[1][3] == 4 and a[2][1]
    # success at the last allowed iteration: bNoMore stays false on that call and is raised by the next
    a, b = _walk_both([1, 2, 3, 4, 40], 60, m, 5, [5, 5])
    assert a == b and a[0][:2] == (4, False) and a[1][:2] == (-1, True)
    # N < minInliers: :144; N == minInliers: one iteration, whose count (at most N) cannot exceed minInliers
    a, b = _walk_both([], 15, m, 0, [5, 5])
    assert a == b and all(e[:2] == (-1, True) for e in a)
    a, b = _walk_both([20], 20, m, 1, [5])
    assert a == b and a[0][:2] == (-1, True) and a[0][4] == 20


def test_max_iterations():
    from cube_slam_amd.sim3_solver import max_iterations
    for N in list(range(3, 130)) + [200, 400, 1000, 5000, 10 ** 6]:  # (the last two: a quotient beyond int, and pow() below 2^-53)
        for min_inl, prob, cap in ((20, 0.99, 300), (6, 0.99, 300), (20, 0.999, 50), (3, 0.5, 300)):
            want = 0 if N < min_inl else R.set_ransac_parameters(prob, min_inl, cap, N)
            assert max_iterations(prob, min_inl, cap, N) == want, (N, min_inl, prob, cap)
    assert max_iterations(0.99, 20, 300, 20) == 1 and max_iterations(0.99, 20, 300, 19) == 0 and max_iterations(0.99, 20, 300, 1000) == 300
    assert max_iterations(0.99, 6, 300, 5000) == 300 and max_iterations(0.5, 3, 300, 10 ** 6) == 300  # the stated rule where the reference's int conversion is undefined


def test_draw_triples():
    from cube_slam_amd.sim3_solver import Sim3Solver
    c = P.solver_case("n63")
    s = Sim3Solver(c["X1"], c["X2"], c["e1"], c["e2"], P.K1, P.K2, c["idx1"], c["mN1"])
    s.SetRansacParameters(P.PROB, P.MIN_INLIERS, P.MAX_ITS)
    rng1, rng2 = np.random.RandomState(9), np.random.RandomState(9)
    got = s.draw_triples(lambda lo, hi: int(rng1.randint(lo, hi + 1)))
    tr = R.IterateTranscription(63, c["mN1"], c["idx1"], 63, c["max_its"])  # (a table of zeros never succeeds: every iteration draws)
    tr.iterate(c["max_its"], np.zeros(c["max_its"], np.int32), None, lambda lo, hi: int(rng2.randint(lo, hi + 1)))
    assert got.tolist() == tr.drawn and len(tr.drawn) == c["max_its"] and all(len(set(t)) == 3 for t in tr.drawn)
    assert np.array_equal(P.draw(63, c["max_its"], 9), got)  # (the patterns' own generator is the same process)


def _python_mirror(names, ctx=None):
    from cube_slam_amd.sim3_solver import Sim3Solver
    out = []
    for nm in names:
        c = P.solver_case(nm)
        s = Sim3Solver(c["X1"], c["X2"], c["e1"], c["e2"], P.K1, P.K2, c["idx1"], c["mN1"], c["fix_scale"], ctx=ctx)
        s.SetRansacParameters(P.PROB, P.MIN_INLIERS, P.MAX_ITS)
        assert s.mRansacMaxIts == c["max_its"]
        if s.mRansacMaxIts:
            s.set_triples(c["triples"])
        out.append(s)
    Sim3Solver.evaluate_many(out, ctx)
    return out


def _same_tables(t, j):
    return np.array_equal(t[0], j["n_inliers"]) and R.same_floats(t[1], j["sRt"]) and np.array_equal(t[2], j["mask"])


def test_python_host_path_equals_restatement():
    solvers = _python_mirror(P.ALL)
    for nm, s in zip(P.ALL, solvers):
        if s.mRansacMaxIts:
            assert _same_tables(s._table, P.judged(nm)), nm


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """The mirror built with nothing of the library, plain and a second time with the sanitizers."""
    d = tmp_path_factory.mktemp("sim3_solver_mirror")
    base = ["g++", "-std=c++17", "-Wall", "-ffp-contract=off", "-DCUBESLAM_HOST_ONLY", "-I", ROOT, os.path.join(ROOT, "tests", "cpp", "sim3_solver_mirror.cpp")]
    subprocess.check_call(base + ["-O2", "-o", str(d / "mirror")])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(d / "mirror_san")])
    return d


def test_gpp_build_of_header_equals_restatement(exes, tmp_path):
    """Every pattern through cubeslam::Sim3Solver without a context and without the library: g++'s build of sim3_host.h over horn_math.h, plain and sanitised, each run as a
    child process.  The output must be, byte for byte, what the restatement's tables, the Python mirror's round-robin over them and the transcription's draw give (no NaN
    occurs in these patterns, so bytes can be compared)."""
    names = P.ALL
    reject = {(names.index(nm), P.first_success(nm)) for nm in ("n21", "n63", "n64_fix", "n65")}
    rng = np.random.RandomState(4)
    c0 = P.solver_case(names[0])
    rnd = [int(rng.randint(0, len(c0["X1"]) - i)) for _ in range(c0["max_its"]) for i in range(3)]
    (tmp_path / "in.bin").write_bytes(P.mirror_input(names, reject, rnd))
    for exe in ("mirror", "mirror_san"):
        r = subprocess.run([str(exes / exe), str(tmp_path / "in.bin"), str(tmp_path / (exe + ".bin")), "host"], capture_output=True, timeout=120)
        assert r.returncode == 0 and r.stderr == b"", (exe, r.stderr.decode())
    tables = [None if not P.solver_case(nm)["max_its"] else (P.judged(nm)["n_inliers"], P.judged(nm)["sRt"], P.judged(nm)["mask"]) for nm in names]
    assert not any(np.isnan(t[1]).any() for t in tables if t is not None)
    log = P.round_robin(_python_mirror(names), reject)
    assert sum(e[1] for e in log) >= 2  # at least one rejected success before the one that ends the loop
    it = iter(rnd)
    from cube_slam_amd.sim3_solver import Sim3Solver
    s0 = Sim3Solver(c0["X1"], c0["X2"], c0["e1"], c0["e2"], P.K1, P.K2, c0["idx1"], c0["mN1"])
    s0.SetRansacParameters(P.PROB, P.MIN_INLIERS, P.MAX_ITS)
    drawn = s0.draw_triples(lambda lo, hi: next(it))
    want = P.mirror_output(names, tables, log, drawn)
    for exe in ("mirror", "mirror_san"):
        assert (tmp_path / (exe + ".bin")).read_bytes() == want, exe
