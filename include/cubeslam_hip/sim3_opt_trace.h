/* cubeslam_hip/sim3_opt_trace.h -- extension of cubeslam_hip.h: what cs_sim3_optimization does on its way, and the exponential under it, alone.
 *   cs_sim3_optimization_trace   cs_sim3_optimization with one record per Levenberg-Marquardt trial and the first linear system of every problem
 *   cs_sim3_exp                  g2o::Sim3(const Vector7d &update) (sim3.h:70-142) of n updates
 * Test probes in the sense of cs_sim3_log: Levenberg-Marquardt reaches the same minimum by many roads, so the end pose cannot tell a wrong Huber factor in H, a wrong
 * initial lambda or a wrong back-up after a rejected trial from the right ones; the trials can.  The kernel is the product's own -- cs_sim3_optimization launches the same
 * one with the trace pointers NULL --, not a copy and not a second instantiation.
 * The main header is unchanged by this file: CS_VERSION and the ABI of its functions stay, this header has a version of its own. */
#ifndef CUBESLAM_HIP_SIM3_OPT_TRACE_H
#define CUBESLAM_HIP_SIM3_OPT_TRACE_H

#include "../cubeslam_hip.h"

#define CS_SIM3_OPT_TRACE_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

/* CS_SIM3_OPT_TRACE_VERSION of the library that is loaded */
int cs_sim3_opt_trace_version(void);

/* One trial of OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:109-149), seven doubles:
 *   stage       0 = optimize(5), 1 = optimize(10 or 5)
 *   iteration   the iteration of that stage, from 0
 *   current_chi currentChi before the trial
 *   temp_chi    activeRobustChi2 after the update as it was computed (before a failed solve replaces it by DBL_MAX)
 *   lambda      the damping the trial solved with
 *   solved      1 where every pivot of the L D L^T was positive, else 0
 *   accepted    1 where the trial was kept (rho > 0 and tempChi finite), 0 where the estimate was restored */
#define CS_SIM3_TRACE_RECORD 7
/* 28 lower-triangle entries of H in row order (H(0,0), H(1,0), H(1,1), H(2,0), ...), the 7 of b, and activeRobustChi2 of that iteration */
#define CS_SIM3_TRACE_SYSTEM 36

/* The first sixteen arguments, the refusals and the three outputs are cs_sim3_optimization's, byte for byte.
 *   trace   [n_problems x max_trials x CS_SIM3_TRACE_RECORD]  the first max_trials trials of every problem in order; records a problem did not reach are zero
 *   n_trials[n_problems]                                      the trials the problem ran, stored or not (0 for a problem without correspondences)
 *   system0 [n_problems x CS_SIM3_TRACE_SYSTEM]               H, b and chi2 of iteration 0 of stage 0, before any damping; zero for a problem without correspondences
 * CS_ERR_BAD_ARG, nothing launched and no output touched: what cs_sim3_optimization refuses, max_trials < 0, and with n_problems > 0 a NULL n_trials or system0, or a
 * NULL trace with max_trials > 0. */
int cs_sim3_optimization_trace(cs_ctx *ctx, int n_problems, const int *corr_off, const double *P1c, const double *P2c, const double *obs1, const double *obs2,
                               const double *inv_sigma2_1, const double *inv_sigma2_2, const double *intrinsics, const double *sim3_in, const float *th2,
                               const uint8_t *fix_scale, double *sim3_out, uint8_t *removed, int *n_inliers, int max_trials, double *trace, int *n_trials, double *system0);

/* update7 [n x 7] = (omega, upsilon, sigma) -> sim3_out8 [n x 8] = tx ty tz qx qy qz qw s, the quaternion as Eigen's Quaterniond(Matrix3d) leaves it (not normalised).
 * CS_ERR_BAD_ARG: n < 0, or n > 0 with a NULL array. */
int cs_sim3_exp(cs_ctx *ctx, int n, const double *update7, double *sim3_out8);

#ifdef __cplusplus
}
#endif
#endif
