// pnp_walk.h -- the host-only rules of PnPsolver (orb_object_slam/src/PnPsolver.cc) that need no arithmetic of a hypothesis: SetRansacParameters (:120-151) and the loop and
// tail of iterate() (:181-255) over the two tables of counts.  One place for cs_pnp_solver_ransac_parameters / cs_pnp_solver_walk (pnpsolver.hip) and for
// cubeslam::PnPsolver with or without the library (host/pnp_solver.hpp).  The iteration count is ransac_iterations (ransac_batch.h), Sim3Solver's too.
#pragma once
#include "ransac_batch.h"

inline void pnp_ransac_parameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon, int N, int *mRansacMinInliers_out, int *mRansacMaxIts_out,
                                  float *mRansacEpsilon_out) {
    int mRansacMinInliers = minInliers;
    float mRansacEpsilon = epsilon;
    int nMinInliers = (int)((float)N * mRansacEpsilon); // int * float: a float product, truncated
    if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    mRansacMinInliers = nMinInliers;
    if (N > 0 && mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N; // (N == 0: iterate returns at :172 and nothing reads the values)
    // (epsilon > 1 where N < mRansacMinInliers: :172 returns before the value is read)
    const int mRansacMaxIts = mRansacMinInliers == N ? 1 : ransac_iterations(probability, mRansacEpsilon, maxIterations);
    *mRansacMinInliers_out = mRansacMinInliers; *mRansacMaxIts_out = mRansacMaxIts; *mRansacEpsilon_out = mRansacEpsilon;
}

inline int pnp_walk(const int *n_inliers, const int *refined_n, int n_hyp, int ransac_max_its, int min_inliers, int *mnIterations, int *mnBestInliers, int *best_hypothesis,
                    int nIterations, int *bNoMore, int *refined) {
    *bNoMore = 0; *refined = 0;
    int nCurrentIterations = 0;
    while (*mnIterations < ransac_max_its || nCurrentIterations < nIterations) { // :181
        if (*mnIterations >= n_hyp) return -2; // the next hypothesis is not in the table: nothing of it is consumed
        nCurrentIterations++;
        const int h = (*mnIterations)++;
        const int mnInliersi = n_inliers[h];
        if (mnInliersi >= min_inliers) { // :208
            if (mnInliersi > *mnBestInliers) { // :211
                *mnBestInliers = mnInliersi;
                *best_hypothesis = h;
            }
            // Refine() runs over mvbBestInliers: the refinement of the latest record, the same again while the best mask has not changed
            if (*best_hypothesis >= 0 && refined_n[*best_hypothesis] > min_inliers) { *refined = 1; return *best_hypothesis; } // :290
        }
    }
    if (*mnIterations >= ransac_max_its) { // :239
        *bNoMore = 1;
        if (*mnBestInliers >= min_inliers && *best_hypothesis >= 0) return *best_hypothesis; // :242, mBestTcw
    }
    return -1;
}
