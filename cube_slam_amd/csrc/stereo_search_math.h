// stereo_search_math.h -- the arithmetic the stereo branches of ORBmatcher::SearchByProjection add to the monocular searches (ORBmatcher.cc:1383-1394, :1433-1438,
// :1459-1465, :104-109): one text for the kernels of match.hip, for the host side of its entry points and for plain C++ under g++ (tests/cpp/stereo_search_driver.cpp).
#pragma once
#include <cmath>

#include "hd.h"

enum { SS_NEITHER = 0, SS_FORWARD = 1, SS_BACKWARD = 2 };

// tlc.z of :1386-1391.  A cv::Mat product is one gemm per row: accumulated in double with k ascending, rounded once.
//   twc[r]  = (float)(-sum_k (double)Rcw[k][r] * (double)tcw[k])           (-Rcw.t() * tcw: the scale -1 is applied to the double sum)
//   tlc_z   = (float)(sum_k (double)Rlw[2][k] * (double)twc[k] + (double)tlw[2])
// Tcw, Tlw: 3 x 4 row-major.
HD float stereo_search_tlc_z(const float *Tcw, const float *Tlw) {
    float twc[3];
    for (int r = 0; r < 3; r++) {
        double acc = 0;
        for (int k = 0; k < 3; k++) acc += (double)Tcw[k * 4 + r] * (double)Tcw[k * 4 + 3];
        twc[r] = (float)(-acc);
    }
    double acc = 0;
    for (int k = 0; k < 3; k++) acc += (double)Tlw[2 * 4 + k] * (double)twc[k];
    return (float)(acc + (double)Tlw[2 * 4 + 3]);
}

// bForward / bBackward of :1393-1394: strict float comparisons with the baseline mb; a monocular search has neither
HD int stereo_search_direction(const float *Tcw, const float *Tlw, float mb, int mono) {
    if (mono) return SS_NEITHER;
    const float z = stereo_search_tlc_z(Tcw, Tlw);
    if (z > mb) return SS_FORWARD;
    if (-z > mb) return SS_BACKWARD;
    return SS_NEITHER;
}

// the level arguments of GetFeaturesInArea at :1433-1438 for a last-frame key point of level o
HD void stereo_search_levels(int direction, int o, int &minLevel, int &maxLevel) {
    if (direction == SS_FORWARD) { minLevel = o; maxLevel = -1; }
    else if (direction == SS_BACKWARD) { minLevel = 0; maxLevel = o; }
    else { minLevel = o - 1; maxLevel = o + 1; }
}

// :1459-1465 and :104-109: a key point with a right coordinate (strictly positive) is no candidate when the query's predicted right coordinate is further from it
// than the window radius
HD bool stereo_search_drops(float ur_query, float u_right, float radius) { return u_right > 0 && fabsf(ur_query - u_right) > radius; }
