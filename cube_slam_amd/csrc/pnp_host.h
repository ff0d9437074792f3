// pnp_host.h -- the problem and correspondence records of cs_pnp_solver_evaluate and its evaluation on one host thread over epnp_math.h: the path of pnpsolver.hip without a
// context, and of cubeslam::PnPsolver built without the library (host/pnp_solver.hpp).  The kernels of pnpsolver.hip make the same statements with a wave as the executor.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "epnp_math.h"

struct PnpProblem { int c0, N, h0, nh, min_inliers, best_in; long w0, s0; double K[4]; }; // first correspondence, their number, first hypothesis, their number, ..., first mask word, first scratch double
struct PnpCorr { float X[3], e, u[2], pad[2]; };                                         // mvP3Dw[i], mvMaxError[i], mvP2D[i]

constexpr int PNP_POINT_DOUBLES = 13; // pws 3, us 2, alphas 4, pcs 3, terms 1
constexpr unsigned PNP_REFINE_QR_SINGULAR = 2u, PNP_RECORD = 4u;

HD void pnp_work_init(EpnpWork *w, const double *K, int n, double *points) {
    w->fu = K[0]; w->fv = K[1]; w->uc = K[2]; w->vc = K[3];
    w->n = n; w->status = 0;
    w->pws = points; w->us = points + 3 * (size_t)n; w->alphas = points + 5 * (size_t)n; w->pcs = points + 9 * (size_t)n; w->terms = points + 12 * (size_t)n;
}

// the host evaluation of the same text
inline void pnp_host_inliers(const PnpProblem &P, const PnpCorr *C, const double *pose, uint32_t *m, int *count) {
    const int W = (P.N + 31) >> 5;
    for (int k = 0; k < W; k++) m[k] = 0;
    int c = 0;
    for (int i = 0; i < P.N; i++)
        if (epnp_is_inlier(pose, pose + 9, P.K, C[i].X, C[i].u, C[i].e)) { m[i >> 5] |= 1u << (i & 31); c++; }
    *count = c;
}

inline void pnp_host_evaluate(const std::vector<PnpProblem> &problems, const std::vector<PnpCorr> &corr, const int *quads, int *n_inliers, double *Rt, uint32_t *status,
                              uint32_t *mask, int *refined_n, double *refined_Rt, uint32_t *refined_mask) {
    const CvxSeq x;
    EpnpWork w;
    std::vector<double> points;
    for (const PnpProblem &P : problems) {
        const PnpCorr *C = corr.data() + P.c0;
        const int W = (P.N + 31) >> 5;
        points.assign((size_t)std::max(P.N, 4) * PNP_POINT_DOUBLES, 0.0);
        int best = P.best_in;
        for (int h = P.h0; h < P.h0 + P.nh; h++) {
            pnp_work_init(&w, P.K, 4, points.data());
            for (int k = 0; k < 4; k++) {
                const PnpCorr &c = C[quads[4 * (size_t)h + k]];
                w.pws[3 * k] = c.X[0]; w.pws[3 * k + 1] = c.X[1]; w.pws[3 * k + 2] = c.X[2];
                w.us[2 * k] = c.u[0]; w.us[2 * k + 1] = c.u[1];
            }
            epnp_compute_pose(x, &w, Rt + 12 * (size_t)h, Rt + 12 * (size_t)h + 9);
            uint32_t *m = mask + P.w0 + (size_t)(h - P.h0) * W;
            pnp_host_inliers(P, C, Rt + 12 * (size_t)h, m, &n_inliers[h]);
            status[h] = w.status;
            refined_n[h] = -1;
            if (!(n_inliers[h] >= P.min_inliers && n_inliers[h] > best)) continue;
            best = n_inliers[h];
            const int n = n_inliers[h];
            pnp_work_init(&w, P.K, n, points.data());
            int k = 0;
            for (int i = 0; i < P.N; i++)
                if ((m[i >> 5] >> (i & 31)) & 1u) {
                    w.pws[3 * (size_t)k] = C[i].X[0]; w.pws[3 * (size_t)k + 1] = C[i].X[1]; w.pws[3 * (size_t)k + 2] = C[i].X[2];
                    w.us[2 * (size_t)k] = C[i].u[0]; w.us[2 * (size_t)k + 1] = C[i].u[1];
                    k++;
                }
            epnp_compute_pose(x, &w, refined_Rt + 12 * (size_t)h, refined_Rt + 12 * (size_t)h + 9);
            pnp_host_inliers(P, C, refined_Rt + 12 * (size_t)h, refined_mask + P.w0 + (size_t)(h - P.h0) * W, &refined_n[h]);
            status[h] |= PNP_RECORD | ((w.status & EPNP_QR_SINGULAR) ? PNP_REFINE_QR_SINGULAR : 0u);
        }
    }
}

// The checks of cs_pnp_solver_evaluate and its records: nullptr, or what is wrong (at[] = the problem and hypothesis it is wrong at, -1 where there is none); nothing is written
// to the caller's arrays.  have_outputs: every output array is given.
inline const char *pnp_build(int n_problems, const int *corr_off, const float *P3Dw, const float *P2D, const float *max_err, const float *K4, const int *min_inliers,
                             const int *best_in, const int *hyp_off, const int *quads, bool have_outputs, std::vector<PnpProblem> &problems, std::vector<PnpCorr> &corr,
                             std::vector<int> &hyp_problem, long *words_out, long *sdoubles_out, long at[2]) {
    at[0] = at[1] = -1;
    if (n_problems < 0) return "n_problems < 0";
    if (n_problems == 0) return nullptr;
    if (!corr_off || !hyp_off || corr_off[0] != 0 || hyp_off[0] != 0) return "offsets that do not start at 0, or a NULL array";
    for (int p = 0; p < n_problems; p++)
        if (corr_off[p + 1] < corr_off[p] || hyp_off[p + 1] < hyp_off[p]) return "offsets that decrease";
    const int NC = corr_off[n_problems], H = hyp_off[n_problems];
    if (!K4 || !min_inliers || !best_in || (NC && (!P3Dw || !P2D || !max_err)) || (H && (!quads || !have_outputs))) return "NULL argument";
    problems.resize((size_t)n_problems);
    hyp_problem.resize((size_t)H);
    long words = 0, sdoubles = 0;
    for (int p = 0; p < n_problems; p++) {
        const int N = corr_off[p + 1] - corr_off[p], nh = hyp_off[p + 1] - hyp_off[p];
        at[0] = p;
        if (nh && N < 4) return "a problem with hypotheses and fewer than 4 correspondences";
        if (nh && min_inliers[p] < 4) return "min_inliers below the minimal set of 4 (SetRansacParameters :136-137)";
        for (int h = hyp_off[p]; h < hyp_off[p + 1]; h++) {
            const int *q = quads + 4 * (size_t)h;
            at[1] = h;
            for (int k = 0; k < 4; k++) {
                if (q[k] < 0 || q[k] >= N) return "a quad index outside its problem (problem, hypothesis)";
                for (int l = 0; l < k; l++) if (q[l] == q[k]) return "two equal indices in a quad (problem, hypothesis)";
            }
            hyp_problem[h] = p;
        }
        at[1] = -1;
        PnpProblem &P = problems[p];
        P.c0 = corr_off[p]; P.N = N; P.h0 = hyp_off[p]; P.nh = nh; P.min_inliers = min_inliers[p]; P.best_in = best_in[p]; P.w0 = words; P.s0 = sdoubles;
        for (int k = 0; k < 4; k++) P.K[k] = K4[4 * (size_t)p + k];
        words += (long)nh * ((N + 31) / 32);
        sdoubles += (long)nh * N * PNP_POINT_DOUBLES; // (a slice per hypothesis, not per record: the records are found on the device.  It grows as H * N -- see cubeslam_hip.h)
    }
    at[0] = -1;
    corr.resize((size_t)NC);
    for (int i = 0; i < NC; i++) {
        PnpCorr &c = corr[i];
        for (int k = 0; k < 3; k++) c.X[k] = P3Dw[3 * (size_t)i + k];
        c.e = max_err[i]; c.u[0] = P2D[2 * (size_t)i]; c.u[1] = P2D[2 * (size_t)i + 1]; c.pad[0] = c.pad[1] = 0;
    }
    *words_out = words; *sdoubles_out = sdoubles;
    return nullptr;
}
