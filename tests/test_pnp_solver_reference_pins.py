"""The library's PnPsolver against the reference's own text.  SetRansacParameters, iterate, Refine, CheckInliers, the EPnP members and the bookkeeping members of
orb_object_slam/src/PnPsolver.cc are cut out of the reference at test time into tmp_path, compiled around tests/cpp/ref_pnp_solver_standins.cpp (a CvMat and a cv::Mat sufficient
for them, the OpenCV calls forwarding to csrc/cv_svd_math.h, RandomInt replaying the pattern's quads) and run as a child process on every pattern of
tests/pnp_solver_patterns.py.  Nothing cut or compiled is written inside the repository.  Required bit for bit on every pattern: mRansacMinInliers / mRansacMaxIts /
mRansacEpsilon; per hypothesis mRi, mti, the count and the mask; per record the refined values; through the scripted Relocalization round-robin of iterate(5) calls with
rejected successes the same matrix-or-none, bNoMore, nInliers, vbInliers, mnIterations, mnBestInliers.  The process's stderr is empty: the reference's "A is singular" branch,
where it leaves X unwritten, is never reached (tests/test_pnp_solver_patterns.py checks the same from the library's status bits).  The reference run is the fixture
tests/golden/pnp_solver.npz: the committed file equals a fresh run byte for byte (PNP_SOLVER_WRITE_GOLDEN=1 rewrites it)."""
import io
import os
import subprocess
import zipfile

import numpy as np
import pytest

from tests import pnp_solver_patterns as P
from tests.test_sim3_restatement_pins import _cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden", "pnp_solver.npz")
pytestmark = pytest.mark.skipif(not os.path.isdir(REF), reason="the pin is to the reference's text under /root/reference")

WANT = ["void PnPsolver::SetRansacParameters(", "cv::Mat PnPsolver::iterate(", "bool PnPsolver::Refine()", "void PnPsolver::CheckInliers()",
        "void PnPsolver::set_maximum_number_of_correspondences(", "void PnPsolver::reset_correspondences(", "void PnPsolver::add_correspondence(",
        "void PnPsolver::choose_control_points(", "void PnPsolver::compute_barycentric_coordinates(", "void PnPsolver::fill_M(", "void PnPsolver::compute_ccs(",
        "void PnPsolver::compute_pcs(", "double PnPsolver::compute_pose(", "void PnPsolver::copy_R_and_t(", "double PnPsolver::dist2(", "double PnPsolver::dot(",
        "double PnPsolver::reprojection_error(", "void PnPsolver::estimate_R_and_t(", "void PnPsolver::solve_for_sign(", "double PnPsolver::compute_R_and_t(",
        "void PnPsolver::find_betas_approx_1(", "void PnPsolver::find_betas_approx_2(", "void PnPsolver::find_betas_approx_3(", "void PnPsolver::compute_L_6x10(",
        "void PnPsolver::compute_rho(", "void PnPsolver::compute_A_and_b_gauss_newton(", "void PnPsolver::gauss_newton(", "void PnPsolver::qr_solve("]
KEYS = ("n_inliers", "Rt", "status", "mask", "refined_n", "refined_Rt", "refined_mask")


def _mirror_script():
    """The script through the Python mirror on the host path -> the calls [(k, outcome)]."""
    solvers = [P.solver(n) for n in P.SCRIPT_NAMES]

    def iterate(k, n):
        s = solvers[k]
        T, nomore, vb, ni = s.iterate(n)
        return T, nomore, vb, ni, s.mnIterations, s.mnBestInliers
    return P.run_script(iterate)


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    d = tmp_path_factory.mktemp("ref_pnp_solver")
    text = open(os.path.join(REF, "orb_object_slam", "src", "PnPsolver.cc")).read()
    (d / "ref_pnp_solver_extracted.inc").write_text("\n\n".join(_cut(text, s) for s in WANT) + "\n")
    exe = str(d / "ref_pnp_solver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-w", "-ffp-contract=off", "-I" + str(d), "-I" + ROOT, "-o", exe, os.path.join(ROOT, "tests", "cpp", "ref_pnp_solver_standins.cpp")])
    calls = _mirror_script()
    (d / "in.bin").write_bytes(P.driver_input(P.SCRIPT_NAMES, [k for k, _ in calls]))
    r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    out = P.driver_output((d / "out.bin").read_bytes(), P.SCRIPT_NAMES, [k for k, _ in calls])
    out["stderr"], out["calls"] = r.stderr.decode(), calls
    return out


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


def test_stderr_empty(reference):
    assert reference["stderr"] == ""


@pytest.mark.parametrize("name", P.SCRIPT_NAMES)
def test_ransac_parameters(reference, name):
    from cube_slam_amd.pnp_solver import ransac_parameters
    c = P.case(name)
    mi, its, eps = reference["tables"][name]["params"]
    if len(c["P3Dw"]) < c["min_inliers"]:
        assert mi == c["min_inliers"]  # (:172 returns before mRansacMaxIts is read; eps > 1 makes its conversion undefined in the reference)
        return
    lp = ransac_parameters(*c["args"][:5], len(c["P3Dw"]))
    assert (mi, its) == (lp[0], lp[1]) == (c["min_inliers"], c["max_its"]) and eps == lp[2] == c["epsilon"]


@pytest.mark.parametrize("name", P.SCRIPT_NAMES)
def test_tables(reference, name):
    """Per hypothesis mRi, mti, count, mask; per record the refined values; which hypotheses are records."""
    if not len(P.case(name)["quads"]):
        return
    t, j = reference["tables"][name], P.judged(name)
    for k in KEYS:
        assert _same(t[k].reshape(j[k].shape), j[k]), k


def test_round_robin(reference):
    """The scripted Relocalization round-robin: the mirror's outcome of every call equals the reference's."""
    assert len(reference["calls"]) > 40
    successes = 0
    for (k, mine), ref in zip(reference["calls"], reference["script"]):
        name = P.SCRIPT_NAMES[k]
        assert (mine[0] is None) == (ref[0] is None), name
        if ref[0] is not None:
            assert mine[0].dtype == np.float32 and mine[0].tobytes() == ref[0].tobytes(), name
            successes += 1
        assert mine[1] == ref[1] and mine[3] == ref[3] and mine[4] == ref[4] and mine[5] == ref[5], (name, mine[1:], ref[1:])
        assert np.array_equal(mine[2], ref[2]), name
    assert successes > 10  # (rejected successes: the calls go on after them)


def _golden_bytes(reference):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:  # (np.savez stamps the time of writing into the archive)
        def put(key, a):
            b = io.BytesIO(); np.lib.format.write_array(b, np.ascontiguousarray(a), version=(1, 0))
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue())
        for name in P.SCRIPT_NAMES:
            t = reference["tables"][name]
            put(name + "/params", np.array([t["params"][0], t["params"][1]], np.int32)); put(name + "/epsilon", np.float32(t["params"][2]))
            for k in KEYS:
                put(name + "/" + k, t[k])
        for i, ((k, _), o) in enumerate(zip(reference["calls"], reference["script"])):
            put("call%03d/solver" % i, np.int32(k)); put("call%03d/Tcw" % i, np.zeros((0, 4), np.float32) if o[0] is None else o[0])
            put("call%03d/state" % i, np.array([o[1], o[3], o[4], o[5]], np.int32)); put("call%03d/vbInliers" % i, np.packbits(o[2]))
    return buf.getvalue()


def test_golden_regenerates_byte_equal(reference):
    fresh = _golden_bytes(reference)
    if os.environ.get("PNP_SOLVER_WRITE_GOLDEN") == "1":
        with open(GOLDEN, "wb") as f:
            f.write(fresh)
    assert len(fresh) < 1 << 20
    assert open(GOLDEN, "rb").read() == fresh
