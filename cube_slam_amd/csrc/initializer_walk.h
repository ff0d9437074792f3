// initializer_walk.h -- the decisions of Initializer::ReconstructF (orb_object_slam/src/Initializer.cc:503-576) and ReconstructH (:695-736) over what CheckRT returned for
// the candidates: their nGood and the cosine at the order statistic of :902-905.  Host only: acosf is taken here, as the reference takes it after the sort.  One place for
// cs_initializer_walk (initializer.hip) and for cubeslam::Initializer with or without the library (host/initializer.hpp).
#pragma once
#include <math.h>

#include <algorithm>

enum { INIT_MODEL_NONE = -1, INIT_MODEL_H = 0, INIT_MODEL_F = 1 };

// parallax = acos(vCosParallax[idx]) * 180 / CV_PI (:905): acos(float) is the float overload, * 180 a float product, / CV_PI a double quotient stored in a float; 0 where
// nGood == 0 (:908)
inline float init_parallax(int nGood, float cosParallax) {
    if (!(nGood > 0)) return 0.f;
    return (float)((double)(acosf(cosParallax) * 180) / 3.1415926535897932384626433832795);
}

// -> the candidate whose R, t, points and vbGood Initialize returns, or -1 (false).  model: which of the two rules; n_cand: 4, 8, or 0 where ReconstructH returned at :604;
// N: the inliers of the chosen model's mask (:477-480 / :582-585).  parallax_out (optional): the parallax the rule compared, 0 where it compared none
inline int init_walk(int model, int n_cand, const int *nGood, const float *cosParallax, int N, float minParallax, int minTriangulated, float *parallax_out) {
    if (parallax_out) *parallax_out = 0.f;
    if (model == INIT_MODEL_F) {
        if (n_cand != 4) return -1;
        const int maxGood = std::max(nGood[0], std::max(nGood[1], std::max(nGood[2], nGood[3]))); // :503
        const int nMinGood = std::max(static_cast<int>(0.9 * N), minTriangulated);                // :508
        int nsimilar = 0;
        for (int k = 0; k < 4; k++)
            if (nGood[k] > 0.7 * maxGood) nsimilar++; // :511-518
        if (maxGood < nMinGood || nsimilar > 1) return -1; // :521
        for (int k = 0; k < 4; k++) // :527-574: the first candidate that reaches maxGood decides
            if (maxGood == nGood[k]) {
                const float parallax = init_parallax(nGood[k], cosParallax[k]);
                if (parallax_out) *parallax_out = parallax;
                return parallax > minParallax ? k : -1;
            }
        return -1;
    }
    if (model == INIT_MODEL_H) {
        if (n_cand != 8) return -1; // :604
        int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
        float bestParallax = -1;
        for (int i = 0; i < 8; i++) { // :704-724
            if (nGood[i] > bestGood) {
                secondBestGood = bestGood;
                bestGood = nGood[i];
                bestSolutionIdx = i;
                bestParallax = init_parallax(nGood[i], cosParallax[i]);
            } else if (nGood[i] > secondBestGood)
                secondBestGood = nGood[i];
        }
        if (parallax_out) *parallax_out = bestParallax;
        if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 * N) return bestSolutionIdx; // :726
        return -1;
    }
    return -1; // no model
}
