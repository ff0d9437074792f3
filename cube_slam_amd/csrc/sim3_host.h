// sim3_host.h -- the problem and correspondence records of cs_sim3_solver_hypotheses, its checks, its evaluation on one host thread over horn_math.h, and the host-only rules
// of Sim3Solver (orb_object_slam/src/Sim3Solver.cc) that need no arithmetic of a hypothesis: SetRansacParameters (:118-133) and the loop of iterate() (:138-205) over the
// table of counts.  One place for sim3solver.hip (its path without a context and its extern "C" forwards) and for cubeslam::Sim3Solver (host/sim3_solver.hpp), with or
// without the library.  The kernel of sim3solver.hip makes the same statement of a hypothesis with a wave as the executor.
#pragma once
#include "horn_math.h"
#include "ransac_batch.h"

struct S3sProblem { int c0, N, h0, fix; long w0; float K8[8]; }; // first correspondence, their number, first hypothesis, mbFixScale, first mask word
struct S3sCorr { float X1[3], e1, X2[3], e2; };                  // mvX3Dc1[i], mvnMaxError1[i], mvX3Dc2[i], mvnMaxError2[i]: two 16-byte loads

HD void s3s_store(const HornSim3 &H, float *o) { // the 13 floats of a hypothesis: ms12i, mR12i, mt12i
    o[0] = H.s;
    for (int k = 0; k < 9; k++) o[1 + k] = H.R[k];
    for (int k = 0; k < 3; k++) o[10 + k] = H.t[k];
}

// The checks of cs_sim3_solver_hypotheses and its records: nullptr, or what is wrong (ransac_batch_build); nothing is written to the caller's arrays.
inline const char *s3s_build(int n_problems, const int *corr_off, const float *X3Dc1, const float *X3Dc2, const float *max_err1, const float *max_err2, const float *K8,
                             const uint8_t *fix_scale, const int *hyp_off, const int *triples, bool have_outputs, std::vector<S3sProblem> &problems, std::vector<S3sCorr> &corr,
                             std::vector<int> &hyp_problem, long *words_out, long at[2]) {
    std::vector<RansacSlot> slots;
    if (const char *what = ransac_batch_build<3>(n_problems, corr_off, hyp_off, triples, K8 && fix_scale, X3Dc1 && X3Dc2 && max_err1 && max_err2, have_outputs, slots, hyp_problem,
                                                 words_out, at))
        return what;
    problems.resize(slots.size());
    for (size_t p = 0; p < slots.size(); p++) {
        S3sProblem &P = problems[p];
        P.c0 = slots[p].c0; P.N = slots[p].N; P.h0 = slots[p].h0; P.fix = fix_scale[p] != 0; P.w0 = slots[p].w0;
        for (int k = 0; k < 8; k++) P.K8[k] = K8[8 * p + k];
    }
    corr.resize(n_problems ? (size_t)corr_off[n_problems] : 0);
    for (size_t i = 0; i < corr.size(); i++) {
        S3sCorr &c = corr[i];
        for (int k = 0; k < 3; k++) { c.X1[k] = X3Dc1[3 * i + k]; c.X2[k] = X3Dc2[3 * i + k]; }
        c.e1 = max_err1[i]; c.e2 = max_err2[i];
    }
    return nullptr;
}

// the host evaluation of the same text
inline void s3s_host_evaluate(const std::vector<S3sProblem> &problems, const std::vector<int> &hyp_problem, const std::vector<S3sCorr> &corr, const int *triples, int *n_inliers,
                              float *sRt, uint32_t *mask) {
    for (size_t h = 0; h < hyp_problem.size(); h++) {
        const S3sProblem &P = problems[hyp_problem[h]];
        const S3sCorr *C = corr.data() + P.c0;
        const S3sCorr &a = C[triples[3 * h]], &b = C[triples[3 * h + 1]], &c = C[triples[3 * h + 2]];
        HornSim3 H;
        horn_sim3(a.X1, b.X1, c.X1, a.X2, b.X2, c.X2, P.fix != 0, &H);
        ransac_host_inliers(P.N, [&](int i) { return horn_is_inlier(H, C[i].X1, C[i].X2, C[i].e1, C[i].e2, P.K8, nullptr); },
                            mask + P.w0 + (h - P.h0) * ransac_words(P.N), &n_inliers[h]);
        s3s_store(H, sRt + 13 * h);
    }
}

inline int s3s_max_iterations(double probability, int min_inliers, int max_iterations, int N) { // SetRansacParameters :118-133
    if (N < min_inliers) return 0; // iterate returns at :144
    if (min_inliers == N) return 1;
    return ransac_iterations(probability, (float)min_inliers / N, max_iterations);
}

inline int s3s_walk(const int *n_inliers, int ransac_max_its, int min_inliers, int *mnIterations, int *mnBestInliers, int *best_hypothesis, int nIterations, int *bNoMore) {
    *bNoMore = 0;
    int nCurrentIterations = 0;
    while (*mnIterations < ransac_max_its && nCurrentIterations < nIterations) { // :156
        nCurrentIterations++;
        const int t = (*mnIterations)++;
        const int mnInliersi = n_inliers[t];
        if (mnInliersi >= *mnBestInliers) { // :181
            *mnBestInliers = mnInliersi;
            *best_hypothesis = t;
            if (mnInliersi > min_inliers) return t; // :190
        }
    }
    if (*mnIterations >= ransac_max_its) *bNoMore = 1; // :201
    return -1;
}
