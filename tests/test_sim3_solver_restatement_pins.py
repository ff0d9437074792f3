"""The judge of the Sim3Solver tests (tests/sim3_solver_restatement.py) against the reference's own text: Sim3Solver::SetRansacParameters, iterate, ComputeCentroid, ComputeSim3,
CheckInliers, Project and FromCameraToImage (orb_object_slam/src/Sim3Solver.cc) are cut out of the reference at test time into tmp_path, compiled there around
tests/cpp/ref_sim3_solver_standins.cpp (a cv::Mat sufficient for them, cv::eigen as a float Jacobi with descending order, cv::Rodrigues as OpenCV's formula over libm, RandomInt
replaying the pattern's triples) and run on the cases of tests/sim3_solver_patterns.py.  Nothing cut or compiled is written inside the repository.

Required: the same mRansacMaxIts; through a scripted LoopClosing::ComputeSim3 round-robin with rejected successes the same outcome of every iterate(5) call -- matrix or none,
bNoMore, nInliers, mnIterations, mnBestInliers and the same vbInliers; the same count and the same inlier set on every hypothesis without a marginal correspondence.

Measured: the two operations the library replaces by stated definitions (cv::eigen, atan2 + cv::Rodrigues) make sRt and the errors differ by construction.  The distance of the
13 floats ms12i, mR12i, mt12i is taken in units of 2^-24 * scale_k / gap, where gap = (lambda_1 - lambda_2) / lambda_1 is the relative gap between the two largest eigenvalues
of N (the conditioning of the triple) and scale_k is 1 for the scale and the rotation and max(1, |O1|, |s O2|) for the translation; the relative distance of the err values,
|err - err_ref| / max(err, err_ref, threshold), in units of 2 * 2^-24 * (lever * (arm / gap + mag) + pixel) / sqrt(max(err, threshold)) (R.err_units: the
rotation's and the float rounding's displacement of the camera-frame point, times pixels per unit of displacement, plus the rounding of the projection).  Their maxima over all hypotheses of
all patterns are recorded as R.D_REF_T12 and R.D_REF_ERR, the bounds are TOL = 10 x those, and the test asserts 0.5 D <= worst <= D so that a drift in either direction shows.
T12's sR and the returned matrix are held to TOL_T12 as well."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sim3_solver_patterns as P
from tests import sim3_solver_restatement as R
from tests.test_sim3_restatement_pins import _cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the restatement is pinned to the reference's text under /root/reference")

WANT = ["void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations)",
        "cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers)", "void Sim3Solver::ComputeCentroid(cv::Mat &P, cv::Mat &Pr, cv::Mat &C)",
        "void Sim3Solver::ComputeSim3(cv::Mat &P1, cv::Mat &P2)", "void Sim3Solver::CheckInliers()",
        "void Sim3Solver::Project(const vector<cv::Mat> &vP3Dw, vector<cv::Mat> &vP2D, cv::Mat Tcw, cv::Mat K)",
        "void Sim3Solver::FromCameraToImage(const vector<cv::Mat> &vP3Dc, vector<cv::Mat> &vP2D, cv::Mat K)"]
FP, IP, BP = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("ref_sim3_solver")
    text = open(os.path.join(REF, "orb_object_slam", "src", "Sim3Solver.cc")).read()
    (d / "ref_sim3_solver_extracted.inc").write_text("\n\n".join(_cut(text, s) for s in WANT) + "\n")
    so = str(d / "libref_sim3_solver.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-ffp-contract=off", "-fPIC", "-shared", "-I" + str(d), "-o", so, os.path.join(ROOT, "tests", "cpp", "ref_sim3_solver_standins.cpp")])
    lib = C.CDLL(so)
    lib.pin_solver_new.restype = C.c_void_p
    lib.pin_solver_new.argtypes = [C.c_int, C.c_int, FP, FP, FP, FP, FP, IP, C.c_int, C.c_double, C.c_int, C.c_int, IP, C.c_int]
    lib.pin_solver_delete.argtypes = [C.c_void_p]
    lib.pin_solver_max_its.argtypes = [C.c_void_p]
    lib.pin_solver_iterate.argtypes = [C.c_void_p, C.c_int, FP, BP, IP]
    lib.pin_solver_last.argtypes = [C.c_void_p, FP, BP, FP]
    return lib


def _new(ref, name):
    c = P.solver_case(name)
    f = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(FP)
    tr = np.ascontiguousarray(c["triples"], np.int32); idx = np.ascontiguousarray(c["idx1"], np.int32)
    assert (c["e1"] == np.floor(c["e1"])).all() and (c["e2"] == np.floor(c["e2"])).all()  # the size_t thresholds of this reference
    return ref.pin_solver_new(len(c["X1"]), c["mN1"], f(c["X1"]), f(c["X2"]), f(c["e1"]), f(c["e2"]), f(c["K8"]), idx.ctypes.data_as(IP), int(c["fix_scale"]), P.PROB, P.MIN_INLIERS,
                              P.MAX_ITS, tr.ctypes.data_as(IP), len(tr))


def _iterate(ref, h, n, mN1):
    T = np.zeros(16, np.float32); vb = np.zeros(mN1, np.uint8); st = np.zeros(4, np.int32)
    found = ref.pin_solver_iterate(h, n, T.ctypes.data_as(FP), vb.ctypes.data_as(BP), st.ctypes.data_as(IP))
    return found, T.reshape(4, 4), vb, st


@pytest.mark.parametrize("name", P.ALL)
def test_max_iterations(ref, name):
    h = _new(ref, name)
    c = P.solver_case(name)
    if c["max_its"]:  # (N < minInliers: iterate returns at :144 and the reference's value is never read)
        assert ref.pin_solver_max_its(h) == c["max_its"]
    ref.pin_solver_delete(h)


def _hypotheses(ref, name):
    """Every hypothesis of the pattern, one iterate(1) each -> the worst distances; counts and inlier sets must be equal where no correspondence is marginal."""
    c, j = P.solver_case(name), P.judged(name)
    marg, infos, hyps, units = P.margins(name)
    N = len(c["X1"])
    h = _new(ref, name)
    worst_t, worst_e, n_clean = 0.0, 0.0, 0
    sRt = np.zeros(13, np.float32); inl = np.zeros(N, np.uint8); err = np.zeros(2 * N, np.float32)
    for t in range(c["max_its"]):
        _iterate(ref, h, 1, c["mN1"])
        cnt = ref.pin_solver_last(h, sRt.ctypes.data_as(FP), inl.ctypes.data_as(BP), err.ctypes.data_as(FP))
        assert not np.isnan(j["sRt"][t]).any() and not np.isnan(sRt).any()
        d = R.t12_distance(j["sRt"][t], sRt, infos[t])
        assert d <= R.TOL_T12, (name, t, d)
        worst_t = max(worst_t, d)
        mine = j["err"][t].astype(np.float64); theirs = err.reshape(2, N).astype(np.float64)
        thr = np.stack([c["e1"], c["e2"]]).astype(np.float64)
        ok = np.isfinite(mine) & np.isfinite(theirs) & np.isfinite(units[t])
        with np.errstate(all="ignore"):
            de = np.where(ok, np.abs(mine - theirs) / np.maximum(np.maximum(mine, theirs), thr) / units[t], 0.0)
        assert de.max() <= R.TOL_ERR, (name, t, float(de.max()))
        worst_e = max(worst_e, float(de.max()))
        if not marg[t].any():
            n_clean += 1
            assert cnt == j["n_inliers"][t] and np.array_equal(inl.astype(bool), R.unpack_mask(j["mask"][t], N)), (name, t)
    ref.pin_solver_delete(h)
    return worst_t, worst_e, n_clean


def test_distances_and_counts(ref):
    worst_t, worst_e = 0.0, 0.0
    for name in P.ALL:
        if not P.solver_case(name)["max_its"]:
            continue
        a, b, n_clean = _hypotheses(ref, name)
        print("%s: %d hypotheses, %d without a marginal correspondence, T12 distance %.3f, err distance %.3f" % (name, P.solver_case(name)["max_its"], n_clean, a, b))
        worst_t, worst_e = max(worst_t, a), max(worst_e, b)
    print("D_REF_T12 = %r, D_REF_ERR = %r" % (worst_t, worst_e))
    assert 0.5 * R.D_REF_T12 <= worst_t <= R.D_REF_T12 and R.TOL_T12 == 10 * R.D_REF_T12
    assert 0.5 * R.D_REF_ERR <= worst_e <= R.D_REF_ERR and R.TOL_ERR == 10 * R.D_REF_ERR


@pytest.mark.parametrize("names,rejected", [(("n65", "n100_no_consensus", "n15_too_few", "n129"), ("n65",)), (("n20", "n21", "n64_fix", "n63", "n200"), ("n21", "n64_fix", "n63"))])
def test_round_robin(ref, names, rejected):
    """LoopClosing::ComputeSim3's while loop over the reference's solvers and over the Python mirror's host path, with the same successes rejected."""
    from cube_slam_amd.sim3_solver import Sim3Solver
    names = list(names)
    reject = {(names.index(nm), P.first_success(nm)) for nm in rejected}
    mine = []
    for nm in names:
        c = P.solver_case(nm)
        s = Sim3Solver(c["X1"], c["X2"], c["e1"], c["e2"], P.K1, P.K2, c["idx1"], c["mN1"], c["fix_scale"])
        s.SetRansacParameters(P.PROB, P.MIN_INLIERS, P.MAX_ITS)
        if s.mRansacMaxIts:
            s.set_triples(c["triples"])
        mine.append(s)
    log = P.round_robin(mine, reject)
    assert sum(e[1] for e in log) >= 2
    hs = [_new(ref, nm) for nm in names]
    k, disc, n_cand, match = 0, [False] * len(names), len(names), False
    while n_cand > 0 and not match:
        for i, nm in enumerate(names):
            if disc[i]:
                continue
            found, T, vb, st = _iterate(ref, hs[i], 5, P.solver_case(nm)["mN1"])
            e = log[k]; k += 1
            hyp = int(st[2]) - 1
            if st[2] > 0:  # no deciding hypothesis may hold a marginal correspondence (tests/test_sim3_solver_patterns.py)
                assert not P.margins(nm)[0][:st[2]].any()
            assert e[:6] == (i, found, int(st[0]), int(st[1]), int(st[2]), int(st[3])), (nm, e[:6], found, st)
            assert e[7] == vb.tobytes()
            if found:
                Tm = np.frombuffer(e[6], np.float32).reshape(4, 4)
                info = P.margins(nm)[1][hyp]
                sc = max(1.0, float(np.abs(Tm[:3, 3]).max()))
                assert np.abs(Tm.astype(np.float64) - T.astype(np.float64)).max() <= R.TOL_T12 * R.EPS24 * 2 * sc / max(R.gap(info), 1e-300)
            if st[0]:
                disc[i] = True; n_cand -= 1
            if found and (i, hyp) not in reject:
                match = True
                break
    assert k == len(log) and match
    for h in hs:
        ref.pin_solver_delete(h)
