// pnp_host.h -- the problem and correspondence records of cs_pnp_solver_evaluate and its evaluation on one host thread over epnp_math.h: the path of pnpsolver.hip without a
// context, and of cubeslam::PnPsolver with or without the library (host/pnp_solver.hpp).  The kernels of pnpsolver.hip make the same statements with a wave as the executor.
// The batch, its checks and the mask layout are ransac_batch.h's, shared with sim3_host.h.
#pragma once
#include "epnp_math.h"
#include "ransac_batch.h"

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
    ransac_host_inliers(P.N, [&](int i) { return epnp_is_inlier(pose, pose + 9, P.K, C[i].X, C[i].u, C[i].e); }, m, count);
}

inline void pnp_host_evaluate(const std::vector<PnpProblem> &problems, const std::vector<PnpCorr> &corr, const int *quads, int *n_inliers, double *Rt, uint32_t *status,
                              uint32_t *mask, int *refined_n, double *refined_Rt, uint32_t *refined_mask) {
    const CvxSeq x;
    EpnpWork w;
    std::vector<double> points;
    for (const PnpProblem &P : problems) {
        const PnpCorr *C = corr.data() + P.c0;
        const int W = ransac_words(P.N);
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
                if (ransac_mask_bit(m, i)) {
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

// The checks of cs_pnp_solver_evaluate and its records: nullptr, or what is wrong (ransac_batch_build); nothing is written to the caller's arrays.  have_outputs: every output
// array is given.
inline const char *pnp_build(int n_problems, const int *corr_off, const float *P3Dw, const float *P2D, const float *max_err, const float *K4, const int *min_inliers,
                             const int *best_in, const int *hyp_off, const int *quads, bool have_outputs, std::vector<PnpProblem> &problems, std::vector<PnpCorr> &corr,
                             std::vector<int> &hyp_problem, long *words_out, long *sdoubles_out, long at[2]) {
    std::vector<RansacSlot> slots;
    if (const char *what = ransac_batch_build<4>(n_problems, corr_off, hyp_off, quads, K4 && min_inliers && best_in, P3Dw && P2D && max_err, have_outputs, slots, hyp_problem,
                                                 words_out, at))
        return what;
    problems.resize(slots.size());
    long sdoubles = 0;
    for (size_t p = 0; p < slots.size(); p++) {
        const RansacSlot &s = slots[p];
        if (s.nh && min_inliers[p] < 4) { at[0] = (long)p; return "min_inliers below the minimal set of 4 (SetRansacParameters :136-137)"; }
        PnpProblem &P = problems[p];
        P.c0 = s.c0; P.N = s.N; P.h0 = s.h0; P.nh = s.nh; P.min_inliers = min_inliers[p]; P.best_in = best_in[p]; P.w0 = s.w0; P.s0 = sdoubles;
        for (int k = 0; k < 4; k++) P.K[k] = K4[4 * p + k];
        sdoubles += (long)s.nh * s.N * PNP_POINT_DOUBLES; // (a slice per hypothesis, not per record: the records are found on the device.  It grows as H * N -- see cubeslam_hip.h)
    }
    corr.resize(n_problems ? (size_t)corr_off[n_problems] : 0);
    for (size_t i = 0; i < corr.size(); i++) {
        PnpCorr &c = corr[i];
        for (int k = 0; k < 3; k++) c.X[k] = P3Dw[3 * i + k];
        c.e = max_err[i]; c.u[0] = P2D[2 * i]; c.u[1] = P2D[2 * i + 1]; c.pad[0] = c.pad[1] = 0;
    }
    *sdoubles_out = sdoubles;
    return nullptr;
}
