// g2o's Levenberg-Marquardt schedule (the vendored core/optimization_algorithm_levenberg.cpp:61-164): the gain ratio, how lambda shrinks and grows, when a trial is
// repeated and the three ways out of an iteration.  Every optimiser of the library follows it -- the two kernels (poseopt.hip, sim3opt.hip) with the struct in registers,
// the three host loops (ba.hip, badyn.hip, posegraph.hip) -- and each keeps its own loop body around these calls: what a trial is, how a state is backed up and
// restored, the statistics.  The initial lambda is the caller's (computeLambdaInit :166-180: tau * max |diag H|, or the user's value).
//
//     LmSchedule lm;
//     for (it ...) {  errors, currentChi, iniChi = currentChi, build the system;  if (it == 0) lm.start(lambda0);
//         lm.begin_iteration();
//         do { back up, solve with lm.lambda, update, tempChi, scale = x . (lambda x + b);  if (!lm.trial(currentChi, tempChi, solved, scale)) restore; } while (lm.retry());
//         if (lm.stop(iniChi, currentChi)) break;
//     }
// Plain C++ as well as device code: tests/cpp/lm_schedule_driver.cpp runs it with g++ against the reference's own text.
#pragma once
#include <cfloat>
#include <cmath>

#include "hd.h"

struct LmSchedule {
    double lambda = 0, ni = 2, rho = 0;
    int nBad = 0, qmax = 0;

    HD void start(double lambda_init) { lambda = lambda_init; ni = 2; nBad = 0; } // iteration 0, :99-103
    HD void begin_iteration() { rho = 0; qmax = 0; }                                // :105-107
    // One trial (:126-148).  `scale` is computeScale()'s sum without the 1e-3.  An accepted trial's chi2 becomes currentChi; a rejected one leaves it.
    HD bool trial(double &currentChi, double tempChi, bool solved, double scale) {
        if (!solved) tempChi = DBL_MAX;
        rho = currentChi - tempChi;
        scale += 1e-3;
        rho /= scale;
        const bool accepted = rho > 0 && std::isfinite(tempChi);
        if (accepted) {
            double alpha = 1. - pow((2 * rho - 1), 3);
            alpha = fmin(alpha, 2. / 3.); // _goodStepUpperScale
            lambda *= fmax(1. / 3., alpha); // _goodStepLowerScale
            ni = 2;
            currentChi = tempChi;
        } else {
            lambda *= ni;
            ni *= 2;
        }
        qmax++;
        return accepted;
    }
    HD bool retry() const { return rho < 0 && qmax < 10; } // :149, _maxTrialsAfterFailure
    // after the trials of an iteration (:151-161): true ends the run
    HD bool stop(double iniChi, double currentChi) {
        if (qmax == 10 || rho == 0) return true;
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
        return nBad >= 3;
    }
};
