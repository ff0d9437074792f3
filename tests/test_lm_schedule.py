"""CPU: the Levenberg-Marquardt schedule every optimiser of the library shares (cube_slam_amd/csrc/lm_schedule.h), compiled with g++ -ffp-contract=off into
tests/cpp/lm_schedule_driver.cpp.
  * Against the reference's own text: the driver runs an LM loop whose schedule is LmSchedule and whose other steps are the oracle's pieces; ref_ba_levenberg /
    ref_badyn_levenberg (oracle/_ref/libref.so) run OptimizationAlgorithmLevenberg::solve / computeLambdaInit / computeScale and SparseOptimizer::optimize as the
    reference vendors them over the same pieces.  The two runs can differ in the schedule alone and must agree to the last bit, on the problems of the two pin tests
    of tests/test_ref_pins.py.
  * Sequences written by hand for the ways out, each with the line of Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp it comes from."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_ref_pins import LEVENBERG_BA_PROBLEMS, LEVENBERG_BADYN_PROBLEMS, levenberg_ba_problem, levenberg_badyn_problem, ref  # noqa: F401 (ref: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = sys.float_info.max


@pytest.fixture(scope="module")
def driver(tmp_path_factory, oracle):
    so = tmp_path_factory.mktemp("lm_schedule") / "lm_schedule_driver.so"
    odir = os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "lm_schedule_driver.cpp"), "-o", str(so),
                           "-L", odir, "-l:liboracle.so", "-Wl,-rpath," + odir, "-Wl,--no-undefined"])
    lib = C.CDLL(str(so))
    lib.lm_driver_ba.restype = C.c_int
    lib.lm_driver_badyn.restype = C.c_int
    lib.lm_new.restype = C.c_void_p
    return lib


def _dp(a):
    return a.ctypes.data_as(C.c_void_p)


def _run_both(fn_ref, fn_drv, p, iters, shapes):
    res = []
    for fn in (fn_ref, fn_drv):
        out = [np.zeros((max(n, 1), k)) for n, k in shapes]
        trials, lam, chi = C.c_int(), C.c_double(), C.c_double()
        done = fn(C.byref(p), iters, *[_dp(a) for a in out], C.byref(trials), C.byref(lam), C.byref(chi))
        res.append((done, trials.value, lam.value, chi.value, [a[:n] for a, (n, _) in zip(out, shapes)]))
    return res


def _same(r, d, seed):
    assert (d[0], d[1]) == (r[0], r[1]), (seed, "iterations, solves", r[:2], d[:2])
    assert d[2] == r[2] and d[3] == r[3], (seed, "lambda, chi2", r[2:4], d[2:4])
    for a, b in zip(r[4], d[4]):
        assert np.array_equal(a, b), seed


def test_schedule_equals_reference_text_object_ba(ref, oracle, driver):
    ref.ref_ba_levenberg.restype = C.c_int
    rejected = 0
    for seed, kw, iters in LEVENBERG_BA_PROBLEMS:
        p = oracle.ba_struct(levenberg_ba_problem(seed, kw))
        r, d = _run_both(ref.ref_ba_levenberg, driver.lm_driver_ba, p, iters, ((p.n_cams, 7), (p.n_points, 3), (p.n_cuboids, 7)))
        _same(r, d, seed)
        rejected += r[1] - r[0]  # the reference's numbers alone: more solves than iterations is a rejected trial
    assert rejected > 0


def test_schedule_equals_reference_text_dynamic_ba(ref, oracle, driver):
    ref.ref_badyn_levenberg.restype = C.c_int
    rejected = 0
    for seed, kw, iters in LEVENBERG_BADYN_PROBLEMS:
        p = oracle.badyn_struct(levenberg_badyn_problem(seed, kw))
        r, d = _run_both(ref.ref_badyn_levenberg, driver.lm_driver_badyn, p, iters, ((p.n_cams, 7), (p.n_objs, 7), (p.n_vels, 2), (p.n_points, 3), (p.n_dpoints, 3)))
        _same(r, d, seed)
        rejected += r[1] - r[0]
    assert rejected > 0


class Lm:
    """LmSchedule through the driver's lm_* functions; currentChi is the caller's variable, as in the loops."""

    def __init__(self, lib, lambda_init, chi):
        self.lib, self.h, self.chi = lib, C.c_void_p(lib.lm_new()), C.c_double(chi)
        lib.lm_start(self.h, C.c_double(lambda_init))

    def begin(self):
        self.lib.lm_begin_iteration(self.h)
        self.ini = self.chi.value

    def trial(self, temp_chi, solved=True, scale=1.0):
        return bool(self.lib.lm_trial(self.h, C.byref(self.chi), C.c_double(temp_chi), int(solved), C.c_double(scale)))

    def retry(self):
        return bool(self.lib.lm_retry(self.h))

    def stop(self):
        return bool(self.lib.lm_stop(self.h, C.c_double(self.ini), self.chi))

    def state(self):
        lam, ni, rho, n_bad, qmax = C.c_double(), C.c_double(), C.c_double(), C.c_int(), C.c_int()
        self.lib.lm_state(self.h, C.byref(lam), C.byref(ni), C.byref(rho), C.byref(n_bad), C.byref(qmax))
        return dict(lam=lam.value, ni=ni.value, rho=rho.value, nBad=n_bad.value, qmax=qmax.value)

    def close(self):
        self.lib.lm_free(self.h)


@pytest.fixture
def lm(driver):
    made = []

    def make(lambda_init, chi):
        made.append(Lm(driver, lambda_init, chi))
        return made[-1]
    yield make
    for m in made:
        m.close()


def test_failed_solve_is_a_rejection(lm):
    # :126-127 `if (! ok2) tempChi=std::numeric_limits<double>::max();` -- a chi2 that would have been accepted is not looked at
    s = lm(1.0, 10.0)
    s.begin()
    assert s.trial(5.0, solved=False, scale=1.0) is False
    st = s.state()
    assert s.chi.value == 10.0 and st["rho"] == (10.0 - DBL_MAX) / (1.0 + 1e-3) and st["lam"] == 2.0 and st["ni"] == 4.0 and st["qmax"] == 1
    assert s.retry()  # :149 rho < 0 && qmax < 10
    assert s.trial(5.0, solved=True, scale=1.0) is True and s.chi.value == 5.0  # the same chi2 behind a solve that succeeded is taken


def test_non_finite_chi2_is_a_rejection(lm):
    # :134 `if (rho>0 && g2o_isfinite(tempChi))`: -inf gives rho = +inf > 0 and is stopped by the second condition alone; nan and +inf already by the first
    for bad in (-math.inf, math.nan, math.inf):
        s = lm(1.0, 10.0)
        s.begin()
        assert s.trial(bad) is False
        st = s.state()
        assert s.chi.value == 10.0 and st["lam"] == 2.0 and st["ni"] == 4.0, bad  # :144-145
    s = lm(1.0, 10.0)
    s.begin()
    s.trial(-math.inf)
    assert s.state()["rho"] == math.inf and not s.retry()  # rho > 0: the trial loop ends (:149) ...
    assert not s.stop()  # ... and the run goes on (:151: neither qmax == 10 nor rho == 0; :155: the first iteration without improvement)


def test_ten_rejections_end_the_iteration_and_the_run(lm):
    # :149 `while (rho<0 && qmax < _maxTrialsAfterFailure->value() ...)` with the constructor's 10 (:52), :151 `if (qmax == _maxTrialsAfterFailure->value() || rho==0) return Terminate;`
    s = lm(3.0, 10.0)
    s.begin()
    for k in range(10):
        assert s.trial(11.0) is False
        assert s.retry() == (k < 9), k
    st = s.state()
    assert st["qmax"] == 10 and st["rho"] < 0 and s.chi.value == 10.0
    assert st["lam"] == 3.0 * 2.0 ** 55 and st["ni"] == 2.0 ** 11  # :144-145 ten times: lambda * 2 * 4 * ... * 1024
    assert s.stop()
    # nine rejections and an acceptance do not end it
    s = lm(3.0, 10.0)
    s.begin()
    for k in range(9):
        assert s.trial(11.0) is False and s.retry()
    assert s.trial(1.0) is True and not s.retry() and s.state()["qmax"] == 10
    assert s.stop()  # (qmax == 10 ends the run whatever the last trial did: the reference's condition reads qmax alone)


def test_rho_zero_ends_the_run(lm):
    # :129-132 rho = (currentChi-tempChi) / (scale + 1e-3) = 0; :134 not accepted; :149 rho < 0 fails: no retry; :151 `|| rho==0`: Terminate
    s = lm(1.0, 10.0)
    s.begin()
    assert s.trial(10.0) is False
    st = s.state()
    assert st["rho"] == 0.0 and st["qmax"] == 1 and st["lam"] == 2.0 and st["ni"] == 4.0
    assert not s.retry() and s.stop()


def test_three_small_improvements_end_the_run(lm):
    # :155-161 `if((iniChi-currentChi)*1e3<iniChi) _nBad++; else _nBad=0;  if(_nBad>=3) return Terminate;`
    s = lm(1.0, 1000.0)

    def iteration(factor):
        s.begin()
        assert s.trial(s.chi.value * factor) is True and not s.retry()
        return s.stop()
    small, good = 1 - 0.5e-3, 0.5
    assert not iteration(small) and s.state()["nBad"] == 1
    assert not iteration(small) and s.state()["nBad"] == 2
    assert not iteration(good) and s.state()["nBad"] == 0  # a good one in between: the count starts again
    assert not iteration(small) and s.state()["nBad"] == 1
    assert not iteration(small) and s.state()["nBad"] == 2
    assert iteration(small) and s.state()["nBad"] == 3
    # the comparison is strict: an improvement of exactly iniChi / 1e3 is a good step
    s = lm(1.0, 1000.0)
    s.begin()
    assert s.trial(999.0) is True and (1000.0 - 999.0) * 1e3 == 1000.0 and not s.stop() and s.state()["nBad"] == 0


def _factor(rho):  # :135-139: alpha = 1 - (2 rho - 1)^3 cropped into [_goodStepLowerScale, _goodStepUpperScale] = [1/3, 2/3] (:49-50)
    alpha = 1. - math.pow(2 * rho - 1, 3)
    return max(1. / 3., min(alpha, 2. / 3.))


def test_lambda_and_ni_after_accept_reject_accept(lm):
    lam0, scale = 0.7, 3.0
    s = lm(lam0, 100.0)
    s.begin()
    # accept with rho = 0.9: alpha = 1 - 0.8^3 = 0.488 lies inside the crop
    t1 = 100.0 - 0.9 * (scale + 1e-3)
    rho1 = (100.0 - t1) / (scale + 1e-3)
    assert s.trial(t1, scale=scale) is True
    st = s.state()
    assert st["rho"] == rho1 and 1. / 3. < _factor(rho1) < 2. / 3. and st["lam"] == lam0 * _factor(rho1) and st["ni"] == 2.0 and s.chi.value == t1  # :135-141
    lam1 = st["lam"]
    # reject twice: lambda *= ni, ni *= 2 (:144-145)
    s.begin()
    assert s.trial(t1 + 1.0, scale=scale) is False and s.retry()
    assert s.state()["lam"] == lam1 * 2.0 and s.state()["ni"] == 4.0
    assert s.trial(t1 + 1.0, scale=scale) is False and s.retry()
    assert s.state()["lam"] == lam1 * 2.0 * 4.0 and s.state()["ni"] == 8.0 and s.chi.value == t1
    # accept with a gain ratio near 1: alpha ~ 0, cropped to 1/3; ni back to 2 (:139-140)
    t3 = t1 - (scale + 1e-3)
    rho3 = (t1 - t3) / (scale + 1e-3)
    assert s.trial(t3, scale=scale) is True and not s.retry()
    st = s.state()
    assert st["rho"] == rho3 and _factor(rho3) == 1. / 3. and st["lam"] == lam1 * 2.0 * 4.0 * (1. / 3.) and st["ni"] == 2.0 and st["qmax"] == 3
    # accept with a small gain ratio: alpha ~ 2, cropped to 2/3
    s.begin()
    t4 = t3 - 0.01 * (scale + 1e-3)
    lam3 = st["lam"]
    assert s.trial(t4, scale=scale) is True
    assert _factor((t3 - t4) / (scale + 1e-3)) == 2. / 3. and s.state()["lam"] == lam3 * (2. / 3.)
