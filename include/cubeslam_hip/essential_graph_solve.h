/* cubeslam_hip/essential_graph_solve.h -- extension of cubeslam_hip.h: the linear solve inside cs_essential_graph_optimize, alone.
 *   cs_essential_graph_solve   one (H + lambda I) x = b of the pose graph's Levenberg-Marquardt trial, from Jacobians and errors the caller supplies
 * A test probe in the sense of cs_sim3_log: the optimiser forgives an inexact step (a trial that still lowers chi2 is accepted), so the sparse block Cholesky is judged
 * here against a dense solve of the same system.  The launches are the optimiser's own (the same host functions issue them in both places), not a copy.
 * The main header is unchanged by this file: CS_VERSION and the ABI of its functions stay, this header has a version of its own. */
#ifndef CUBESLAM_HIP_ESSENTIAL_GRAPH_SOLVE_H
#define CUBESLAM_HIP_ESSENTIAL_GRAPH_SOLVE_H

#include "../cubeslam_hip.h"

#define CS_ESSENTIAL_GRAPH_SOLVE_VERSION 1

#ifdef __cplusplus
extern "C" {
#endif

/* CS_ESSENTIAL_GRAPH_SOLVE_VERSION of the library that is loaded */
int cs_essential_graph_solve_version(void);

/* J [m x 14 x 7] in eg_linearize's layout, J[(e * 14 + side * 7 + d) * 7 + k] = d err_k / d update_d of the vertex on `side` of edge e (side 0 = edge_i, 1 = edge_j), and
 * err [m x 7] are copied into the handle's own Jacobian and error buffers; then the optimiser's assembly (H_ii = sum J^T J, H_ij, b = -sum J^T err, each in edge order), its
 * factorisation of H + lambda I over the handle's launch list and its back substitution run once.
 *   x_out [n x 7]   the solution by vertex (not by position in the elimination order); the fixed vertex's row is zero
 *   *status         0, or 1 where a 7 x 7 diagonal block met a pivot that is not > 0 (NaN included): the optimiser's "solve failed".  x_out is then whatever the
 *                   substitutions made of it, finite or not
 * The fixed vertex's side of J is not read: the incidence and slot lists never name it, so whatever stands there (eg_linearize writes zeros) has no effect.
 * The handle's estimates are not touched, and a later cs_essential_graph_optimize rebuilds everything this call wrote.
 * CS_ERR_BAD_ARG, with nothing launched: a NULL argument, or a handle of another context.  A lambda that is not finite is not an error: *status and x_out say what came of it. */
int cs_essential_graph_solve(cs_ctx *ctx, cs_essential_graph *eg, const double *J, const double *err, double lambda, double *x_out, int *status);

#ifdef __cplusplus
}
#endif
#endif
