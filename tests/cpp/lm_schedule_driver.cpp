// TEST INFRASTRUCTURE (never linked into the product): cube_slam_amd/csrc/lm_schedule.h compiled with g++ -ffp-contract=off, as the host loops of the library see it.
//  * lm_driver_ba / lm_driver_badyn: a Levenberg-Marquardt run whose schedule is LmSchedule and whose every other step is the oracle's piece -- the same calls the
//    stand-ins of oracle/ref_shim/ref_levenberg_api.cpp make for the reference's own solve() text, so the two runs can differ in the schedule alone
//    (tests/test_lm_schedule.py compares them bit for bit);
//  * lm_*: the struct's members one by one, for sequences written by hand.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../cube_slam_amd/csrc/lm_schedule.h"
#include "../../oracle/oracle.h"

namespace {
// SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve over an open handle; returns the iterations done
int run(orc_ba_handle *h, int iterations, int *trials, double *lambda_final, double *chi2_final) {
    int P = 0, L = 0, done = 0;
    orc_ba_sizes(h, &P, &L);
    LmSchedule lm;
    *trials = 0;
    for (int it = 0; it < iterations; it++) {
        orc_ba_compute_errors(h);
        double currentChi = orc_ba_robust_chi2(h);
        const double iniChi = currentChi;
        orc_ba_build_system(h);
        if (it == 0) { // computeLambdaInit: tau * max |diag H| over the vertices in index order
            double mx = 0;
            for (int k = 0; k < P + L; k++) for (int j = 0, dim = orc_ba_block_dim(h, k); j < dim; j++) mx = std::max(std::fabs(orc_ba_hessian_diag(h, k, j)), mx);
            lm.start(1e-5 * mx);
        }
        lm.begin_iteration();
        do {
            orc_ba_push(h);
            const bool solved = orc_ba_solve(h, lm.lambda) != 0;
            (*trials)++;
            orc_ba_update(h);
            orc_ba_compute_errors(h);
            const double tempChi = orc_ba_robust_chi2(h);
            long n = 0;
            const double *x = orc_ba_x(h, &n), *b = orc_ba_b(h);
            double scale = 0; // computeScale
            for (long j = 0; j < n; j++) scale += x[j] * (lm.lambda * x[j] + b[j]);
            if (lm.trial(currentChi, tempChi, solved, scale)) orc_ba_discard_top(h);
            else orc_ba_pop(h);
        } while (lm.retry());
        done = it + 1;
        if (lm.stop(iniChi, currentChi)) break;
    }
    orc_ba_compute_errors(h);
    *chi2_final = orc_ba_robust_chi2(h);
    *lambda_final = lm.lambda;
    return done;
}
} // namespace

extern "C" {
int lm_driver_ba(const orc_ba_problem *p, int iterations, double *cam_pose, double *points, double *cuboid_pose, int *trials, double *lambda_final, double *chi2_final) {
    orc_ba_handle *h = orc_ba_open(p);
    const int done = run(h, iterations, trials, lambda_final, chi2_final);
    orc_ba_read(h, cam_pose, points, cuboid_pose);
    orc_ba_close(h);
    return done;
}
int lm_driver_badyn(const orc_badyn_problem *p, int iterations, double *cam_pose, double *obj_pose, double *vel, double *points, double *dpoints, int *trials, double *lambda_final,
                    double *chi2_final) {
    orc_ba_handle *h = orc_badyn_open(p);
    const int done = run(h, iterations, trials, lambda_final, chi2_final);
    orc_badyn_read(h, cam_pose, obj_pose, vel, points, dpoints);
    orc_ba_close(h);
    return done;
}

LmSchedule *lm_new() { return new LmSchedule(); }
void lm_free(LmSchedule *lm) { delete lm; }
void lm_start(LmSchedule *lm, double lambda_init) { lm->start(lambda_init); }
void lm_begin_iteration(LmSchedule *lm) { lm->begin_iteration(); }
int lm_trial(LmSchedule *lm, double *currentChi, double tempChi, int solved, double scale) { return lm->trial(*currentChi, tempChi, solved != 0, scale) ? 1 : 0; }
int lm_retry(const LmSchedule *lm) { return lm->retry() ? 1 : 0; }
int lm_stop(LmSchedule *lm, double iniChi, double currentChi) { return lm->stop(iniChi, currentChi) ? 1 : 0; }
void lm_state(const LmSchedule *lm, double *lambda, double *ni, double *rho, int *nBad, int *qmax) { *lambda = lm->lambda; *ni = lm->ni; *rho = lm->rho; *nBad = lm->nBad; *qmax = lm->qmax; }
}
